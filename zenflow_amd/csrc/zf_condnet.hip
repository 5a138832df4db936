// Conditioning networks on the device: the `Phi` of examples/deep_set.ipynb
// (cells `class NNBlock` / `class Phi` / `class DeepSetFlow` / `loss_fn_2`),
//   BatchNorm -> (Dense, act) x depth -> Dense -> Dropout -> sum (or max) over each set,
// forward, reverse (parameter and input gradients for a given d loss / d c) and the
// optimiser update, behind zf_condnet_* (include/zenflow_amd.h); and the
// standalone segment sum / mean / max / broadcast / repeat, zf_segment_*.
//
// The Dense layers, the weight-gradient trees, BatchNorm and the optimiser
// are the trainer's, included as they are (zf_gemm.h, zf_reduce.h,
// zf_train_kernels.h, zf_optim.h): this unit instantiates its own copies of
// those kernels, the trainer's code object is untouched.  New here: the
// segmented reduction over ragged sets, its reverse, the repeat, and dropout.
//
// Data parallelism (zf_condnet_set_comm, zf_condnet_forward_shard): a rank
// holds whole sets, B of the global pass's Bg element rows from row_base on.
// Every leaf layout and GEMM form follows Bg, the ranks' fp64 subtree roots are
// all-gathered and combined by the top of the leaf tree (cn_combine; the
// gradient close), as the trainer does; pooling is per set and exchanges
// nothing; the dropout mask is indexed by the global row.
#include "zf_gemm.h"
#include "zf_internal.h"
#include "zf_optim.h"
#include "zf_random.h"
#include "zf_reduce.h"
#include "zf_train_kernels.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace zf {
namespace {

constexpr int kSegChunk = ZF_SEG_CHUNK;
constexpr int64_t kSegMaxSets = 1ll << 24;
constexpr int64_t kSegMaxRows = (1ll << 31) - 1;  // the row -> set index is int32; the launch grids stay below 2^31
constexpr int kPlanThreads = 1024;

// The dropout rule of include/zenflow_amd.h: d = keep(i, f) ? v / (1 - rate) : 0.
// keep_prob = (float)1 - rate is formed once on the host.  i is the row of the
// global pass: the kernels add row_base (0 on one device and in zf_segment_*).
template <bool DROP>
__device__ __forceinline__ float drop_apply(float v, unsigned long long seed, long long i, int f, float rate,
                                            float keep_prob) {
#pragma clang fp contract(off)
  if (!DROP) return v;
  const float u = u01_co(philox_at(seed, i, f, ZF_DROPOUT_STREAM).v[ZF_DROPOUT_WORD]);
  return u >= rate ? v / keep_prob : 0.f;
}

// ---- the plan of one batch of sets: one block over the S + 1 offsets ---------
// o[s] = max over j <= s of clamp(off[j], 0, rows)   (non-decreasing, inside h)
// cb[s] = chunks of the sets before s, cb[S] = all chunks; set s has
// ceil((o[s+1] - o[s]) / kSegChunk) of them, and none when it has at most
// `skip` rows (0: an empty set; 1 above the first level: a set that is down
// to one row is finished).  Thread t owns the offsets
// [t per, (t + 1) per); the threads' slice maxima / chunk counts are scanned
// through LDS (Hillis-Steele, 10 steps).
__global__ __launch_bounds__(kPlanThreads) void seg_plan_kernel(const long long* __restrict__ off, long long S,
                                                                long long rows, long long skip,
                                                                long long* __restrict__ o,
                                                                long long* __restrict__ cb) {
  __shared__ long long sc[2][kPlanThreads];
  auto chunks_of = [&](long long len) { return len <= skip ? 0ll : (len + kSegChunk - 1) / kSegChunk; };
  const int t = threadIdx.x;
  const long long n = S + 1, per = (n + kPlanThreads - 1) / kPlanThreads;
  const long long i0 = min(n, (long long)t * per), i1 = min(n, i0 + per);
  long long m = 0;
  for (long long i = i0; i < i1; ++i) m = max(m, min(max(off[i], 0ll), rows));
  // inclusive prefix maximum over the threads
  int cur = 0;
  sc[0][t] = m;
  __syncthreads();
  for (int d = 1; d < kPlanThreads; d *= 2) {
    sc[cur ^ 1][t] = t >= d ? max(sc[cur][t], sc[cur][t - d]) : sc[cur][t];
    cur ^= 1;
    __syncthreads();
  }
  long long run = t > 0 ? sc[cur][t - 1] : 0;
  __syncthreads();
  for (long long i = i0; i < i1; ++i) {
    run = max(run, min(max(off[i], 0ll), rows));
    o[i] = run;
  }
  __syncthreads();  // o[] of the whole block is visible: a slice's last set reads its neighbour's first offset
  long long cnt = 0;
  for (long long i = i0; i < i1 && i < S; ++i) cnt += chunks_of(o[i + 1] - o[i]);
  cur = 0;
  sc[0][t] = cnt;
  __syncthreads();
  for (int d = 1; d < kPlanThreads; d *= 2) {
    sc[cur ^ 1][t] = t >= d ? sc[cur][t] + sc[cur][t - d] : sc[cur][t];
    cur ^= 1;
    __syncthreads();
  }
  long long base = t > 0 ? sc[cur][t - 1] : 0;
  for (long long i = i0; i < i1; ++i) {
    cb[i] = base;
    if (i < S) base += chunks_of(o[i + 1] - o[i]);
  }
}

// ---- one level: one wave per chunk ------------------------------------------------
// The s with cb[s] <= c < cb[s + 1], found by the whole wave: 64 probes per
// step (cb is non-decreasing, cb[0] <= c < cb[S]).
__device__ __forceinline__ long long seg_find_set(const long long* __restrict__ cb, long long S, long long c,
                                                  int lane) {
  long long lo = 0, hi = S;
  while (hi - lo > 1) {
    const long long step = (hi - lo + 63) / 64;
    const long long at = min(lo + lane * step, hi);
    const int k = __popcll(__ballot(cb[at] <= c));  // lanes 0 .. k - 1 hold (k >= 1: lane 0 probes lo)
    hi = min(lo + k * step, hi);
    lo = lo + (k - 1) * step;
  }
  return lo;
}

// Chunk c belongs to the set s = seg_find_set(c); it covers the set's rows
// [k kSegChunk, min(n, (k + 1) kSegChunk)), k = c - cb[s].  Lane (j, f) =
// (lane / F, lane % F), j < R = 64 / F, adds rows j, j + R, ... of the chunk
// in order; lane (0, f) then adds the R lane partials in order j = 0 .. R - 1.
// Eight rows' loads are in flight before their (in-order) adds.  The sum of a
// set's only chunk is the set's result, row s of `out` (zeroed before: empty
// sets have no chunk); every other chunk's sum is row c of `part`, a row of
// the next level (the last level, where no set has two chunks, has no `part`).
// With set_index the lanes of column 0 also record the set of every row they read.
template <bool DROP>
__global__ __launch_bounds__(256) void seg_chunk_sum_kernel(const float* __restrict__ h, int F, long long S,
                                                            const long long* __restrict__ o,
                                                            const long long* __restrict__ cb, float rate,
                                                            float keep_prob, unsigned long long seed,
                                                            long long row_base, float* __restrict__ part,
                                                            float* __restrict__ out, int* __restrict__ set_index) {
#pragma clang fp contract(off)
  __shared__ float red[4][64];
  // (the wave's number as a scalar: the chunk, its set, its first row and its mask row then live in SGPRs)
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long long c = (long long)blockIdx.x * 4 + w;
  const bool live = c < cb[S];
  const int R = 64 / F, j = lane / F, f = lane - j * F;
  float acc = 0.f;
  long long s = 0;
  bool only = false;
  if (live) {
    s = seg_find_set(cb, S, c, lane);
    only = cb[s + 1] - cb[s] == 1;
    if (j < R) {
      const long long r0 = o[s] + (c - cb[s]) * kSegChunk;  // first row of the chunk
      const int len = (int)min((long long)kSegChunk, o[s + 1] - r0);
      const long long d0 = r0 + row_base;  // its row in the dropout mask
      int r = j;
      for (; r + 7 * R < len; r += 8 * R) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = h[(r0 + r + u * R) * F + f];
#pragma unroll
        for (int u = 0; u < 8; ++u) acc = acc + drop_apply<DROP>(v[u], seed, d0 + r + u * R, f, rate, keep_prob);
      }
      for (; r < len; r += R) acc = acc + drop_apply<DROP>(h[(r0 + r) * F + f], seed, d0 + r, f, rate, keep_prob);
      if (set_index && f == 0)
        for (int q = j; q < len; q += R) set_index[r0 + q] = (int)s;
    }
  }
  red[w][lane] = acc;
  __syncthreads();
  if (live && lane < F) {
    float v = red[w][lane];
    for (int q = 1; q < R; ++q) v = v + red[w][q * F + lane];
    if (only) out[s * F + lane] = v;
    else if (part) part[c * F + lane] = v;
  }
}

// ---- the reverse: g_h[i, f] = gc[set(i), f] keep(i, f) / (1 - rate) ---------------
// idx NULL: every row is its own set (the per-row network: dropout's reverse alone).
template <bool DROP>
__global__ void seg_bcast_kernel(const float* __restrict__ gc, const int* __restrict__ idx, long long rows, int F,
                                 long long S, float rate, float keep_prob, unsigned long long seed,
                                 long long row_base, float* __restrict__ g) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= rows * F) return;
  const long long i = t / F;
  const int f = (int)(t - i * F);
  const long long s = idx ? (long long)idx[i] : i;
  const float v = (s >= 0 && s < S) ? gc[s * F + f] : 0.f;
  g[t] = drop_apply<DROP>(v, seed, i + row_base, f, rate, keep_prob);
}

// ---- the repeat: out[i, :] = c[set(i), :] from the clamped offsets ------------------
// One block per kRepRows consecutive rows.  Thread r finds the set of the
// block's row r by bisection over o[0 .. S] (the last s with o[s] <= i; a row
// before o[0] or from o[S] on is in no set: -1), leaves it in LDS and, with
// set_index, in memory; the block then writes its kRepRows * F floats in
// element order.  The work of a row does not depend on its set's length.
constexpr int kRepRows = 256;
__global__ __launch_bounds__(kRepRows) void seg_repeat_kernel(const float* __restrict__ c, int F, long long S,
                                                              const long long* __restrict__ o, long long rows,
                                                              float* __restrict__ out, int* __restrict__ set_index) {
  __shared__ int sidx[kRepRows];
  const int t = threadIdx.x;
  const long long r0 = (long long)blockIdx.x * kRepRows, i = r0 + t;
  int s = -1;
  if (i < rows && i >= o[0] && i < o[S]) {
    long long lo = 0, hi = S;  // o[lo] <= i < o[hi]
    while (hi - lo > 1) {
      const long long mid = lo + (hi - lo) / 2;
      if (o[mid] <= i) lo = mid;
      else hi = mid;
    }
    s = (int)lo;
  }
  sidx[t] = s;
  if (set_index && i < rows) set_index[i] = s;
  __syncthreads();
  const int n = (int)min((long long)kRepRows, rows - r0) * F;
  for (int e = t; e < n; e += kRepRows) {
    const int r = e / F, f = e - r * F;
    const int q = sidx[r];
    out[r0 * F + e] = q >= 0 ? c[(long long)q * F + f] : 0.f;
  }
}

// ---- mean and max over each set (jnp.mean / jnp.max in Phi.__call__) -----------------
// The mask of drop_apply alone: the max's reverse needs d(i, f) and the
// dropout reverse of the same element, one Philox draw for both.
template <bool DROP>
__device__ __forceinline__ bool drop_keep(unsigned long long seed, long long i, int f, float rate) {
  if (!DROP) return true;
  return u01_co(philox_at(seed, i, f, ZF_DROPOUT_STREAM).v[ZF_DROPOUT_WORD]) >= rate;
}

// max(a, b) with a NaN in either making the result NaN (fmaxf drops NaNs): a
// NaN accumulator stays (both comparisons are false), a NaN b replaces it.
__device__ __forceinline__ float nan_max(float a, float b) { return (b > a || b != b) ? b : a; }

// d is a maximal entry of a (set, column) whose maximum is m; for a NaN maximum the NaN entries are.
__device__ __forceinline__ bool is_tie(float d, float m) { return d == m || (m != m && d != d); }

// One level of the max: seg_chunk_sum_kernel with nan_max in place of the
// addition and -inf in place of +0 (a chunk has at least one row, so no -inf
// of the start survives; the maximum is exact, the order of the comparisons
// changes no bit but the sign of a zero).  Dropped entries are zeros that
// take part (Dropout, then the pooling).
template <bool DROP>
__global__ __launch_bounds__(256) void seg_chunk_max_kernel(const float* __restrict__ h, int F, long long S,
                                                            const long long* __restrict__ o,
                                                            const long long* __restrict__ cb, float rate,
                                                            float keep_prob, unsigned long long seed,
                                                            long long row_base, float* __restrict__ part,
                                                            float* __restrict__ out, int* __restrict__ set_index) {
#pragma clang fp contract(off)
  __shared__ float red[4][64];
  // (the wave's number as a scalar: the chunk, its set, its first row and its mask row then live in SGPRs)
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long long c = (long long)blockIdx.x * 4 + w;
  const bool live = c < cb[S];
  const int R = 64 / F, j = lane / F, f = lane - j * F;
  float acc = -INFINITY;
  long long s = 0;
  bool only = false;
  if (live) {
    s = seg_find_set(cb, S, c, lane);
    only = cb[s + 1] - cb[s] == 1;
    if (j < R) {
      const long long r0 = o[s] + (c - cb[s]) * kSegChunk;  // first row of the chunk
      const int len = (int)min((long long)kSegChunk, o[s + 1] - r0);
      const long long d0 = r0 + row_base;  // its row in the dropout mask
      int r = j;
      for (; r + 7 * R < len; r += 8 * R) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = h[(r0 + r + u * R) * F + f];
#pragma unroll
        for (int u = 0; u < 8; ++u)
          acc = nan_max(acc, drop_apply<DROP>(v[u], seed, d0 + r + u * R, f, rate, keep_prob));
      }
      for (; r < len; r += R) acc = nan_max(acc, drop_apply<DROP>(h[(r0 + r) * F + f], seed, d0 + r, f, rate, keep_prob));
      if (set_index && f == 0)
        for (int q = j; q < len; q += R) set_index[r0 + q] = (int)s;
    }
  }
  red[w][lane] = acc;
  __syncthreads();
  if (live && lane < F) {
    float v = red[w][lane];
    for (int q = 1; q < R; ++q) v = nan_max(v, red[w][q * F + lane]);
    if (only) out[s * F + lane] = v;
    else if (part) part[c * F + lane] = v;
  }
}

// The tie count of the max, first pass: one wave per chunk of h's rows (the
// first level's o and cb), lanes (j, f) as above count the chunk's entries
// with d(i, f) == m[s, f] in int32.  A set's only chunk writes count[s, f]
// (zeroed before: empty sets), every other chunk row c of `cpart`.
template <bool DROP>
__global__ __launch_bounds__(256) void seg_chunk_ties_kernel(const float* __restrict__ h, int F, long long S,
                                                             const long long* __restrict__ o,
                                                             const long long* __restrict__ cb, float rate,
                                                             float keep_prob, unsigned long long seed,
                                                             long long row_base, const float* __restrict__ m,
                                                             int* __restrict__ cpart, int* __restrict__ count) {
  __shared__ int red[4][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long long c = (long long)blockIdx.x * 4 + w;
  const bool live = c < cb[S];
  const int R = 64 / F, j = lane / F, f = lane - j * F;
  int acc = 0;
  long long s = 0;
  bool only = false;
  if (live) {
    s = seg_find_set(cb, S, c, lane);
    only = cb[s + 1] - cb[s] == 1;
    if (j < R) {
      const long long r0 = o[s] + (c - cb[s]) * kSegChunk;
      const int len = (int)min((long long)kSegChunk, o[s + 1] - r0);
      const long long d0 = r0 + row_base;
      const float top = m[s * F + f];
      int r = j;
      for (; r + 7 * R < len; r += 8 * R) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = h[(r0 + r + u * R) * F + f];
#pragma unroll
        for (int u = 0; u < 8; ++u)
          acc += is_tie(drop_apply<DROP>(v[u], seed, d0 + r + u * R, f, rate, keep_prob), top) ? 1 : 0;
      }
      for (; r < len; r += R)
        acc += is_tie(drop_apply<DROP>(h[(r0 + r) * F + f], seed, d0 + r, f, rate, keep_prob), top) ? 1 : 0;
    }
  }
  red[w][lane] = acc;
  __syncthreads();
  if (live && lane < F) {
    int v = red[w][lane];
    for (int q = 1; q < R; ++q) v += red[w][q * F + lane];
    if (only) count[s * F + lane] = v;
    else cpart[c * F + lane] = v;
  }
}

// Second pass: one wave per set of more than one chunk adds the set's chunk
// counts, rows cb[s] .. cb[s + 1] - 1 of `cpart` (integers: any order).
__global__ __launch_bounds__(256) void seg_ties_sum_kernel(const int* __restrict__ cpart, int F, long long S,
                                                           const long long* __restrict__ cb,
                                                           int* __restrict__ count) {
  __shared__ int red[4][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long long s = (long long)blockIdx.x * 4 + w;
  const int R = 64 / F, j = lane / F, f = lane - j * F;
  const long long c0 = s < S ? cb[s] : 0, n = s < S ? cb[s + 1] - c0 : 0;
  int acc = 0;
  if (n > 1 && j < R)
    for (long long q = j; q < n; q += R) acc += cpart[(c0 + q) * F + f];
  red[w][lane] = acc;
  __syncthreads();
  if (n > 1 && lane < F) {
    int v = red[w][lane];
    for (int q = 1; q < R; ++q) v += red[w][q * F + lane];
    count[s * F + lane] = v;
  }
}

// The mean's finish on the sum's result: out[s, f] / (float)n_s, one IEEE
// division (an empty set keeps its +0), and n_s as the count of every column.
__global__ void seg_mean_finish_kernel(float* __restrict__ out, int F, long long S, const long long* __restrict__ o,
                                       int* __restrict__ count) {
#pragma clang fp contract(off)
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= S * F) return;
  const long long s = t / F;
  const long long n = o[s + 1] - o[s];
  if (n > 0) out[t] = out[t] / (float)n;
  if (count) count[t] = (int)n;
}

// ---- their reverse --------------------------------------------------------------------
// mean: g_d[i, f] = gc[s, f] / (float)n_s;  max: gc[s, f] / (float)t[s, f] on
// the maximal entries d(i, f) == m[s, f] (an even split among ties, d
// recomputed from h and the mask), 0 elsewhere; then dropout's reverse, as
// seg_bcast_kernel applies it.  Rows in no set (and a count of 0) give 0.
template <bool DROP, bool MAX>
__global__ void seg_pool_bcast_kernel(const float* __restrict__ gc, const int* __restrict__ idx, long long rows,
                                      int F, long long S, float rate, float keep_prob, unsigned long long seed,
                                      long long row_base, const float* __restrict__ h,
                                      const float* __restrict__ m, const int* __restrict__ count,
                                      float* __restrict__ g) {
#pragma clang fp contract(off)
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= rows * F) return;
  const long long i = t / F;
  const int f = (int)(t - i * F);
  const long long s = idx[i];
  float v = 0.f;
  const bool keep = drop_keep<DROP>(seed, i + row_base, f, rate);
  if (s >= 0 && s < S) {
    const int n = count[s * F + f];
    bool on = n > 0;
    if (MAX && on) {
      const float hv = h[t];
      const float d = DROP ? (keep ? hv / keep_prob : 0.f) : hv;
      on = is_tie(d, m[s * F + f]);
    }
    if (on) v = gc[s * F + f] / (float)n;
  }
  g[t] = DROP ? (keep ? v / keep_prob : 0.f) : v;
}

// The levels of one segment sum: level 0 sums the chunks of h's rows, level
// k > 0 those of level k - 1's chunk sums (a set's chunk sums are consecutive
// rows of `part`, its offsets the chunk counts cb: again sets of rows), until
// no set has more than one: 512^levels >= rows.  A set that is down to one
// chunk is finished (its sum goes to `out`) and takes no part in the levels
// above, so the level count, which follows the batch's rows, changes no bit.
inline int seg_levels(long long rows) {
  int n = 1;
  for (long long cap = kSegChunk; cap < rows; cap *= kSegChunk) ++n;
  return n;
}
inline long long seg_max_chunks(long long rows, long long S) { return rows / kSegChunk + S + 1; }
// Workspace: per level o[S + 1], cb[S + 1] (int64); per level but the last its chunk sums.
inline long long seg_ws_bytes(long long rows, long long S, int F) {
  const int L = seg_levels(rows);
  long long bytes = 2ll * L * (S + 1) * (long long)sizeof(long long), r = rows;
  for (int k = 0; k + 1 < L; ++k) {
    r = seg_max_chunks(r, S);
    bytes += r * F * (long long)sizeof(float);
  }
  return bytes;
}

int seg_check(const void* a, const void* b, const void* c, long long rows, int F, long long S, float rate) {
  if (!a || !b || !c) return einval("segment: NULL argument");
  if (rows < 0 || S < 0 || F < 1) return einval("segment: rows %lld, sets %lld, F %d", rows, S, F);
  if (!(rate >= 0.f && rate < 1.f)) return einval("segment: dropout rate %g outside [0, 1)", (double)rate);
  if (F > 64) return enotsup("segment: more than 64 columns");
  if (S > kSegMaxSets) return enotsup("segment: more than 2^24 sets");
  if (rows > kSegMaxRows) return enotsup("segment: more than 2^31 - 1 rows");
  return ZF_OK;
}

// mx: the levels of the max (seg_chunk_max_kernel) over the same plan, workspace and grids.
// row_base: row 0 of h in the dropout mask's numbering (a data-parallel shard's first global row; 0 otherwise).
int seg_reduce_launch(const float* h, long long rows, int F, const long long* off, long long S, float rate,
                      unsigned long long seed, long long row_base, float* out, int* set_index, void* ws, bool mx,
                      hipStream_t st) {
  if (set_index) ZF_TRY_HIP(hipMemsetAsync(set_index, 0xff, (size_t)rows * sizeof(int), st));  // -1: in no set
  if (S == 0) return ZF_OK;
  ZF_TRY_HIP(hipMemsetAsync(out, 0, (size_t)S * F * sizeof(float), st));  // empty sets
  const int L = seg_levels(rows);
  const float kp = 1.0f - rate;
  long long* o = (long long*)ws;
  float* part = (float*)(o + 2ll * L * (S + 1));
  const float* in = h;
  long long in_rows = rows;
  for (int k = 0; k < L; ++k, o += 2 * (S + 1)) {
    long long* cb = o + (S + 1);
    hipLaunchKernelGGL(seg_plan_kernel, dim3(1), dim3(kPlanThreads), 0, st, off, S, in_rows, (long long)(k > 0), o,
                       cb);
    ZF_CHECK_LAUNCH("seg_plan_kernel");
    const long long chunks = seg_max_chunks(in_rows, S);
    const dim3 grid((unsigned)((chunks + 3) / 4));
    float* dst = k + 1 == L ? nullptr : part;
    const bool drop = k == 0 && rate > 0.f;
    auto* const kernel = mx ? (drop ? seg_chunk_max_kernel<true> : seg_chunk_max_kernel<false>)
                            : (drop ? seg_chunk_sum_kernel<true> : seg_chunk_sum_kernel<false>);
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, in, F, S, (const long long*)o, (const long long*)cb, rate, kp,
                       seed, row_base, dst, out, k == 0 ? set_index : nullptr);
    ZF_CHECK_LAUNCH(mx ? "seg_chunk_max_kernel" : "seg_chunk_sum_kernel");
    in = part;
    in_rows = chunks;
    off = cb;
    part += chunks * F;
  }
  return ZF_OK;
}

int seg_sum_launch(const float* h, long long rows, int F, const long long* off, long long S, float rate,
                   unsigned long long seed, float* out, int* set_index, void* ws, hipStream_t st) {
  return seg_reduce_launch(h, rows, F, off, S, rate, seed, 0, out, set_index, ws, false, st);
}

int seg_bcast_launch(const float* gc, const int* idx, long long rows, int F, long long S, float rate,
                     unsigned long long seed, long long row_base, float* g, hipStream_t st) {
  if (rows == 0) return ZF_OK;
  const float kp = 1.0f - rate;
  if (rate > 0.f)
    hipLaunchKernelGGL(seg_bcast_kernel<true>, dim3(blocks_for(rows * F)), dim3(256), 0, st, gc, idx, rows, F, S, rate,
                       kp, seed, row_base, g);
  else
    hipLaunchKernelGGL(seg_bcast_kernel<false>, dim3(blocks_for(rows * F)), dim3(256), 0, st, gc, idx, rows, F, S,
                       rate, kp, seed, row_base, g);
  ZF_CHECK_LAUNCH("seg_bcast_kernel");
  return ZF_OK;
}

// The plan kernel for the clamped offsets (the workspace's first level: o, cb), then the repeat.
int seg_repeat_launch(const float* c, long long S, int F, const long long* off, long long rows, float* out,
                      int* set_index, void* ws, hipStream_t st) {
  if (rows == 0) return ZF_OK;
  if (S == 0) {  // no set: every row is in none
    ZF_TRY_HIP(hipMemsetAsync(out, 0, (size_t)rows * F * sizeof(float), st));
    if (set_index) ZF_TRY_HIP(hipMemsetAsync(set_index, 0xff, (size_t)rows * sizeof(int), st));
    return ZF_OK;
  }
  long long* o = (long long*)ws;
  hipLaunchKernelGGL(seg_plan_kernel, dim3(1), dim3(kPlanThreads), 0, st, off, S, rows, 0ll, o, o + (S + 1));
  ZF_CHECK_LAUNCH("seg_plan_kernel");
  hipLaunchKernelGGL(seg_repeat_kernel, dim3((unsigned)((rows + kRepRows - 1) / kRepRows)), dim3(kRepRows), 0, st, c,
                     F, S, (const long long*)o, rows, out, set_index);
  ZF_CHECK_LAUNCH("seg_repeat_kernel");
  return ZF_OK;
}

inline bool seg_pool_known(int pool) { return pool == ZF_POOL_SUM || pool == ZF_POOL_MEAN || pool == ZF_POOL_MAX; }

// The reduction's workspace and, for the max, the first level's chunk tie counts behind it.
inline long long seg_pool_ws_bytes(long long rows, long long S, int F, int pool) {
  long long bytes = seg_ws_bytes(rows, S, F);
  if (pool == ZF_POOL_MAX) bytes += seg_max_chunks(rows, S) * F * (long long)sizeof(int);
  return bytes;
}

// sum: seg_sum_launch.  mean: the same launches, then the divide.  max: the
// max's levels, then (with count) the two tie-count passes over the first
// level's plan, which the levels leave in the workspace.
int seg_pool_launch(const float* h, long long rows, int F, const long long* off, long long S, int pool, float rate,
                    unsigned long long seed, long long row_base, float* out, int* set_index, int* count, void* ws,
                    hipStream_t st) {
  const int rc =
      seg_reduce_launch(h, rows, F, off, S, rate, seed, row_base, out, set_index, ws, pool == ZF_POOL_MAX, st);
  if (rc || S == 0 || pool == ZF_POOL_SUM) return rc;
  const long long* o = (const long long*)ws;
  const long long* cb = o + (S + 1);
  if (pool == ZF_POOL_MEAN) {
    hipLaunchKernelGGL(seg_mean_finish_kernel, dim3(blocks_for(S * F)), dim3(256), 0, st, out, F, S, o, count);
    ZF_CHECK_LAUNCH("seg_mean_finish_kernel");
    return ZF_OK;
  }
  if (!count) return ZF_OK;
  ZF_TRY_HIP(hipMemsetAsync(count, 0, (size_t)S * F * sizeof(int), st));  // empty sets
  int* cpart = (int*)((char*)ws + seg_ws_bytes(rows, S, F));
  const float kp = 1.0f - rate;
  const dim3 grid((unsigned)((seg_max_chunks(rows, S) + 3) / 4));
  if (rate > 0.f)
    hipLaunchKernelGGL(seg_chunk_ties_kernel<true>, grid, dim3(256), 0, st, h, F, S, o, cb, rate, kp, seed, row_base,
                       (const float*)out, cpart, count);
  else
    hipLaunchKernelGGL(seg_chunk_ties_kernel<false>, grid, dim3(256), 0, st, h, F, S, o, cb, rate, kp, seed, row_base,
                       (const float*)out, cpart, count);
  ZF_CHECK_LAUNCH("seg_chunk_ties_kernel");
  hipLaunchKernelGGL(seg_ties_sum_kernel, dim3((unsigned)((S + 3) / 4)), dim3(256), 0, st, (const int*)cpart, F, S, cb,
                     count);
  ZF_CHECK_LAUNCH("seg_ties_sum_kernel");
  return ZF_OK;
}

int seg_pool_bcast_launch(const float* gc, const int* idx, long long rows, int F, long long S, int pool, float rate,
                          unsigned long long seed, long long row_base, const float* h, const float* m,
                          const int* count, float* g, hipStream_t st) {
  if (pool == ZF_POOL_SUM) return seg_bcast_launch(gc, idx, rows, F, S, rate, seed, row_base, g, st);
  if (rows == 0) return ZF_OK;
  const float kp = 1.0f - rate;
  const bool mx = pool == ZF_POOL_MAX, drop = rate > 0.f;
  auto* const kernel = mx ? (drop ? seg_pool_bcast_kernel<true, true> : seg_pool_bcast_kernel<false, true>)
                          : (drop ? seg_pool_bcast_kernel<true, false> : seg_pool_bcast_kernel<false, false>);
  hipLaunchKernelGGL(kernel, dim3(blocks_for(rows * F)), dim3(256), 0, st, gc, idx, rows, F, S, rate, kp, seed,
                     row_base, h, m, count, g);
  ZF_CHECK_LAUNCH("seg_pool_bcast_kernel");
  return ZF_OK;
}

}  // namespace
}  // namespace zf

// ============================================================================
struct zf_condnet {
  zf_condnet_desc desc;
  int in = 0, F = 0, L = 0;  // input columns, output columns, hidden layers
  int64_t nat_floats = 0, rows_max = 0, sets_max = 0;
  std::vector<void*> bufs;
  float* d_nat = nullptr;
  float* d_grad = nullptr;
  unsigned char* d_mask = nullptr;
  double* d_g64 = nullptr;   // fp64 gradient accumulator (blob layout)
  float* d_x = nullptr;      // [rows_max][in] the pass's input (without BatchNorm: layer 0's input)
  float* d_uhat = nullptr;   // [rows_max][in] BatchNorm's normalised input
  float* d_ubn = nullptr;    // [rows_max][in] BatchNorm's output
  float* d_mean = nullptr;   // [in]
  float* d_rstd = nullptr;   // [in]
  std::vector<float*> Z, H;  // [rows_max][hidden[l]]
  float* d_h = nullptr;      // [rows_max][F] the last Dense's output
  float* d_gl = nullptr;     // [rows_max][F] its gradient
  float* d_ga = nullptr;     // [rows_max][widest layer] gradients, in turn
  float* d_gb = nullptr;
  float* d_gu = nullptr;     // [rows_max][in] d / d BatchNorm's output
  int* d_set = nullptr;      // [rows_max] set(i)
  float* d_pool = nullptr;   // [sets_max][F] the pooled result (max: the reverse compares against it)
  int* d_cnt = nullptr;      // [sets_max][F] max: its tie counts
  void* d_segws = nullptr;
  double* d_leaf = nullptr;
  double* d_leaf2 = nullptr;
  double* d_roots = nullptr;
  float* d_ws = nullptr;     // split-K partials (kWsFloats)
  double* d_ws2 = nullptr;
  float* d_split = nullptr;  // split-set GEMM partials (kSplitFloats)
  // the pending train-mode pass
  bool pending = false;
  int64_t pend_rows = 0, pend_sets = 0;
  int64_t pend_global = 0, pend_base = 0;  // the global pass's rows, this rank's first row in it
  uint64_t pend_seed = 0;
  // data parallelism (zf_condnet_set_comm): world 1 is one device
  zf_comm_desc comm{0, 1, nullptr, nullptr};
  double* d_gath = nullptr;  // [world][max(nat_floats, 256)] the ranks' fp64 roots
  int64_t gath_bytes = 0;
  // optimiser chain
  zf::ChainPlan plan;
  std::vector<void*> opt_bufs;
  unsigned char* d_dmask = nullptr;
  double* d_nleaf = nullptr;
  int n_nleaf = 0;
  zf::OptScalars* d_osc = nullptr;
  bool have_grad = false;
  bool train_ready = false;  // cn_ensure_train has run
  int wmax = 0;              // the widest layer
};

namespace zf {
namespace {

template <typename T>
T* cn_alloc(zf_condnet* h, int64_t n, int& rc) {
  if (rc) return nullptr;
  void* p = nullptr;
  const hipError_t e = hipMalloc(&p, (size_t)(n > 0 ? n : 1) * sizeof(T));
  if (e != hipSuccess) {
    rc = hip_status(e, "zf_condnet alloc");
    return nullptr;
  }
  h->bufs.push_back(p);
  return (T*)p;
}

void cn_free_chain(zf_condnet* h) {
  for (void* p : h->opt_bufs) (void)hipFree(p);
  h->opt_bufs.clear();
  h->d_dmask = nullptr;
  h->d_nleaf = nullptr;
  h->d_osc = nullptr;
}

int cn_opt_alloc(zf_condnet* h, void** p, size_t bytes) {
  *p = nullptr;
  ZF_TRY_HIP(hipMalloc(p, bytes ? bytes : 1));
  h->opt_bufs.push_back(*p);
  ZF_TRY_HIP(hipMemset(*p, 0, bytes ? bytes : 1));
  return ZF_OK;
}

// The buffers only a train-mode pass, its reverse and the optimiser read:
// pre-activations, gradients, the row -> set index, the reduction leaves and
// the split-K workspace (128 MB).  Allocated by the first call that needs
// them, so a handle that only evaluates (ConditionNet.apply) stays small.
int cn_ensure_train(zf_condnet* h) {
  if (h->train_ready) return ZF_OK;
  const int64_t B = h->rows_max, need = h->nat_floats;
  const int wmax = h->wmax;
  int rc = ZF_OK;
  h->d_grad = cn_alloc<float>(h, need, rc);
  h->d_g64 = cn_alloc<double>(h, need, rc);
  h->d_x = cn_alloc<float>(h, B * h->in, rc);
  h->d_uhat = cn_alloc<float>(h, B * h->in, rc);
  h->d_gu = cn_alloc<float>(h, B * h->in, rc);
  for (int l = 0; l < h->L; ++l) h->Z.push_back(cn_alloc<float>(h, B * h->desc.hidden[l], rc));
  h->d_gl = cn_alloc<float>(h, B * h->F, rc);
  h->d_ga = cn_alloc<float>(h, B * wmax, rc);
  h->d_gb = cn_alloc<float>(h, B * wmax, rc);
  h->d_set = cn_alloc<int>(h, B, rc);
  if (h->desc.pool == ZF_POOL_MAX) {
    h->d_pool = cn_alloc<float>(h, h->sets_max * h->F, rc);
    h->d_cnt = cn_alloc<int>(h, h->sets_max * h->F, rc);
  }
  h->d_leaf = cn_alloc<double>(h, (int64_t)kLeafCap * 128, rc);
  h->d_leaf2 = cn_alloc<double>(h, (int64_t)(kLeafCap / kMaxLeaves) * 128, rc);
  h->d_roots = cn_alloc<double>(h, 256, rc);
  h->d_ws = cn_alloc<float>(h, kWsFloats, rc);
  h->d_ws2 = cn_alloc<double>(h, kWsFloats / kMaxLeaves, rc);
  if (rc) return rc;
  ZF_TRY_HIP(hipMemset(h->d_g64, 0, (size_t)need * sizeof(double)));
  ZF_TRY_HIP(hipMemset(h->d_grad, 0, (size_t)need * sizeof(float)));
  h->train_ready = true;
  return ZF_OK;
}

// Install a validated chain: zeroed moment arrays, the decay mask, the norm
// leaves and the device scalars (count 0).  The caller has synchronised.
int cn_install_chain(zf_condnet* h, const ChainPlan& plan, const unsigned char* decay_mask) {
  cn_free_chain(h);
  ChainPlan p = plan;
  const size_t need = (size_t)h->nat_floats;
  int rc = ZF_OK;
  for (int k = 0; k < p.n_slots && !rc; ++k) rc = cn_opt_alloc(h, (void**)&p.args.slot[k], need * sizeof(float));
  if (!rc && p.masked) {
    rc = cn_opt_alloc(h, (void**)&h->d_dmask, need);
    if (!rc) rc = hip_status(hipMemcpy(h->d_dmask, decay_mask, need, hipMemcpyHostToDevice), "zf_condnet decay mask");
  }
  h->n_nleaf = (int)((h->nat_floats + kNormSpan - 1) / kNormSpan);
  if (!rc) rc = cn_opt_alloc(h, (void**)&h->d_nleaf, (size_t)std::max(1, h->n_nleaf) * sizeof(double));
  if (!rc) rc = cn_opt_alloc(h, (void**)&h->d_osc, sizeof(OptScalars));
  if (rc) {
    cn_free_chain(h);
    return rc;
  }
  h->plan = p;
  return ZF_OK;
}

// zf_optim_desc's (n)adamw as the chain optax.adamw builds.
zf_optim_chain adamw_chain(const zf_optim_desc& o) {
  zf_optim_chain c;
  std::memset(&c, 0, sizeof(c));
  c.n_stages = 3;
  c.stages[0].kind = ZF_OPT_SCALE_BY_ADAM;
  c.stages[0].flags = o.nesterov ? ZF_OPT_FLAG_NESTEROV : 0;
  c.stages[0].p[0] = o.b1;
  c.stages[0].p[1] = o.b2;
  c.stages[0].p[2] = o.eps;
  c.stages[1].kind = ZF_OPT_ADD_DECAYED_WEIGHTS;
  c.stages[1].p[0] = o.weight_decay;
  c.stages[2].kind = ZF_OPT_SCALE_BY_LEARNING_RATE;
  c.stages[2].sched.kind = ZF_SCHED_CONSTANT;
  c.stages[2].sched.n_segments = 1;
  c.stages[2].sched.seg_kind[0] = ZF_SCHED_CONSTANT;
  c.stages[2].sched.p[0][0] = (double)o.learning_rate;
  return c;
}

inline int layer_out(const zf_condnet* h, int l) { return l == h->L ? h->F : h->desc.hidden[l]; }
inline int layer_in(const zf_condnet* h, int l) { return l == 0 ? h->in : h->desc.hidden[l - 1]; }

// Data parallelism, as the trainer's dp_combine: this rank's tree roots (n
// doubles, in place) -> the global ones: all-gather every rank's roots,
// combine them by the top of the leaf tree.  Nothing to do on one device.
int cn_combine(zf_condnet* h, double* roots, long long n, hipStream_t st) {
  const int W = h->comm.world;
  if (W <= 1) return ZF_OK;
  if ((int64_t)n * (int64_t)sizeof(double) * W > h->gath_bytes) return einval("all-gather buffer too small");
  const int rc = h->comm.allgather(h->comm.ctx, roots, h->d_gath, (size_t)n * sizeof(double), st);
  if (rc) return rc;
  return launch_tree_cols((const double*)h->d_gath, W, n, roots, st);
}

// BatchNorm of the pass's B rows, this rank's shard of Bg: train mode on the
// statistics of all Bg rows (the trainer's multi-launch path: leaf sums in row
// order, the fp64 leaf tree, the ranks' roots combined, bn_stats_kernel,
// bn_apply_kernel), eval mode on the stored ones.
int cn_batchnorm(zf_condnet* h, const float* x, int B, long long Bg, int train, int update_stats, hipStream_t st) {
  const int DC = h->in;
  float* bn = h->d_nat + h->desc.off_bn;  // [mean, var, scale, bias]
  if (!train) {
    // (D = dc = in_dim, no rotation, no condition: U is x itself)
    hipLaunchKernelGGL(bn_eval_fwd_kernel, dim3(blocks_for((int64_t)B * DC)), dim3(256), 0, st, x,
                       (const float*)nullptr, (const float*)bn, h->d_ubn, h->d_rstd, B, DC, 0, 0, DC, 0);
    ZF_CHECK_LAUNCH("bn_eval_fwd_kernel");
    return ZF_OK;
  }
  const Leaves lbn = leaves_for(B, Bg, h->comm.world, kBnLeafCap);
  hipLaunchKernelGGL(leaf_colsums_kernel, dim3(blocks_for((int64_t)lbn.n * DC)), dim3(256), 0, st, x,
                     (const float*)nullptr, B, DC, lbn.rows, lbn.n, h->d_leaf);
  ZF_CHECK_LAUNCH("leaf_colsums_kernel");
  int rc = launch_tree_cols(h->d_leaf, lbn.n, 2 * DC, h->d_roots, st, h->d_leaf2);
  if (rc) return rc;
  if ((rc = cn_combine(h, h->d_roots, 2 * DC, st))) return rc;
  hipLaunchKernelGGL(bn_stats_kernel, dim3(1), dim3(64), 0, st, (const double*)h->d_roots,
                     (const double*)(h->d_roots + DC), Bg, DC, bn, h->d_mean, h->d_rstd, update_stats);
  ZF_CHECK_LAUNCH("bn_stats_kernel");
  hipLaunchKernelGGL(bn_apply_kernel, dim3(blocks_for((int64_t)B * DC)), dim3(256), 0, st, x,
                     (const float*)h->d_mean, (const float*)h->d_rstd, (const float*)(bn + 2 * DC),
                     (const float*)(bn + 3 * DC), h->d_uhat, h->d_ubn, B, DC);
  ZF_CHECK_LAUNCH("bn_apply_kernel");
  return ZF_OK;
}

// The Dense chain: `in` -> Z[l], H[l] = act(Z[l]) -> out_last (B rows of F).
// Eval mode keeps no pre-activations.  Bg picks the GEMM forms.
int cn_dense_fwd(zf_condnet* h, const float* in, int B, long long Bg, int train, float* out_last, hipStream_t st) {
  const float* nat = h->d_nat;
  for (int l = 0; l <= h->L; ++l) {
    const bool last = l == h->L;
    const int in_w = layer_in(h, l), out_w = layer_out(h, l);
    float* C = last ? out_last : (train ? h->Z[l] : nullptr);
    const int rc = gemm(false, Bg, B, out_w, in_w, in, in_w, nat + h->desc.off_w[l], out_w, C, out_w, st, kEpiBias,
                        nat + h->desc.off_b[l], last ? nullptr : h->H[l], nullptr, h->desc.act, h->d_split,
                        kSplitFloats);
    if (rc) return rc;
    if (!last) in = h->H[l];
  }
  return ZF_OK;
}

// The pass on this rank's B rows, rows [row_base, row_base + B) of a global pass of Bg (one device: B, 0).
int cn_forward(zf_condnet* h, const float* x, int B, long long Bg, long long row_base, const long long* off,
               long long S, int train, int update_stats, unsigned long long seed, float* c_out, hipStream_t st) {
  const bool pool = h->desc.pool != ZF_POOL_NONE;
  const float rate = train ? h->desc.dropout : 0.f;
  int rc;
  const float* in0 = x;
  if (h->desc.batch_norm) {
    if ((rc = cn_batchnorm(h, x, B, Bg, train, update_stats, st))) return rc;
    in0 = h->d_ubn;
  } else if (train) {  // layer 0's weight gradient reads its input after the caller's x may be gone
    ZF_TRY_HIP(hipMemcpyAsync(h->d_x, x, (size_t)B * h->in * sizeof(float), hipMemcpyDeviceToDevice, st));
    in0 = h->d_x;
  }
  // per-row output without dropout: the last Dense writes c_out itself
  float* hl = (!pool && rate == 0.f) ? c_out : h->d_h;
  if ((rc = cn_dense_fwd(h, in0, B, Bg, train, hl, st))) return rc;
  if (pool) {
    rc = seg_pool_launch(hl, B, h->F, off, S, h->desc.pool, rate, seed, row_base, c_out, train ? h->d_set : nullptr,
                         train ? h->d_cnt : nullptr, h->d_segws, st);
    if (rc || !train || h->desc.pool != ZF_POOL_MAX) return rc;
    // the reverse reads the maxima after the caller's c_out may be gone
    ZF_TRY_HIP(hipMemcpyAsync(h->d_pool, c_out, (size_t)S * h->F * sizeof(float), hipMemcpyDeviceToDevice, st));
    return ZF_OK;
  }
  if (rate > 0.f) return seg_bcast_launch(hl, nullptr, B, h->F, B, rate, seed, row_base, c_out, st);
  return ZF_OK;
}

// The reverse pass: gc -> the gradient of the last Dense's output (through the
// pooling and dropout), the Dense chain last layer first (weight and bias
// gradients queued into the fp64 accumulator, input gradients through the
// activation), BatchNorm's scale and bias, then the cast to fp32.  With gx_out
// the chain goes on to the network's input: the first layer's input-gradient
// GEMM (without BatchNorm, straight into gx_out) or BatchNorm's train-mode
// reverse on the column sums the scale and bias gradients reduce anyway.
int cn_backward(zf_condnet* h, const float* gc, float* grad_out, float* gx_out, hipStream_t st) {
  const int B = (int)h->pend_rows, W = h->comm.world;
  const long long Bg = h->pend_global, row_base = h->pend_base;
  const bool pool = h->desc.pool != ZF_POOL_NONE;
  const float rate = h->desc.dropout;
  int rc;
  const float* gout = gc;
  if (pool) {
    rc = seg_pool_bcast_launch(gc, h->d_set, B, h->F, h->pend_sets, h->desc.pool, rate, h->pend_seed, row_base,
                               h->d_h, h->d_pool, h->d_cnt, h->d_gl, st);
    if (rc) return rc;
    gout = h->d_gl;
  } else if (rate > 0.f) {
    if ((rc = seg_bcast_launch(gc, nullptr, B, h->F, B, rate, h->pend_seed, row_base, h->d_gl, st))) return rc;
    gout = h->d_gl;
  }
  WgradQueue wq;
  wq.tb.count = 0;
  wq.gq.count = 0;
  int which = 0;
  for (int l = h->L; l >= 0; --l) {
    const int in_w = layer_in(h, l), out_w = layer_out(h, l);
    const float* hin = l == 0 ? (h->desc.batch_norm ? h->d_ubn : h->d_x) : h->H[l - 1];
    const int cap =
        pow2floor(std::min<int64_t>(kLeafCap, std::max<int64_t>(1, kWsFloats / ((int64_t)(in_w + 1) * out_w))));
    rc = wgrad_deferred(wq, in_w, out_w, B, leaves_for(B, Bg, W, cap), hin, gout, h->d_g64 + h->desc.off_w[l],
                        h->d_g64 + h->desc.off_b[l], h->d_ws, h->d_ws2, st);
    if (rc) return rc;
    if (l == 0 && !h->desc.batch_norm && !gx_out) break;  // d / d x is not asked for
    float* const gin = l == 0 ? (h->desc.batch_norm ? h->d_gu : gx_out) : (which ? h->d_gb : h->d_ga);
    if ((rc = wgrad_before_write(wq, gin, st))) return rc;  // a deferred dW GEMM still reads it
    rc = gemm(true, Bg, B, in_w, out_w, gout, out_w, h->d_nat + h->desc.off_w[l], out_w, gin, in_w, st,
              l > 0 ? kEpiDSwish : kEpiNone, nullptr, nullptr, l > 0 ? h->Z[l - 1] : nullptr, h->desc.act, h->d_split,
              kSplitFloats);
    if (rc) return rc;
    gout = gin;
    which ^= 1;
  }
  if ((rc = wgrad_flush(wq, st))) return rc;
  if (h->desc.batch_norm) {
    // scale / bias: the sums of gUbn * Uhat and gUbn over the rows
    const int DC = h->in;
    const Leaves lbn = leaves_for(B, Bg, W, kBnLeafCap);
    double* gbn = h->d_g64 + h->desc.off_bn;
    hipLaunchKernelGGL(leaf_colsums_kernel, dim3(blocks_for((int64_t)lbn.n * DC)), dim3(256), 0, st,
                       (const float*)h->d_gu, (const float*)h->d_uhat, B, DC, lbn.rows, lbn.n, h->d_leaf);
    ZF_CHECK_LAUNCH("leaf_colsums_kernel");
    if ((rc = launch_tree_cols(h->d_leaf, lbn.n, 2 * DC, h->d_roots, st, h->d_leaf2))) return rc;
    ZF_TRY_HIP(hipMemcpyAsync(gbn + 3 * DC, h->d_roots, DC * sizeof(double), hipMemcpyDeviceToDevice, st));
    ZF_TRY_HIP(hipMemcpyAsync(gbn + 2 * DC, h->d_roots + DC, DC * sizeof(double), hipMemcpyDeviceToDevice, st));
    if (gx_out) {
      // d / d x: the batch terms are those two sums over all Bg rows of the pass (padding rows are in the
      // statistics).  The scale / bias slots above hold this rank's roots (the gradient close adds the ranks');
      // the reverse formula takes the global ones.
      if ((rc = cn_combine(h, h->d_roots, 2 * DC, st))) return rc;
      hipLaunchKernelGGL(bn_bwd_kernel, dim3(blocks_for((int64_t)B * DC)), dim3(256), 0, st, (const float*)h->d_gu,
                         (const float*)h->d_uhat, (const float*)(h->d_nat + h->desc.off_bn + 2 * DC),
                         (const float*)h->d_rstd, (const double*)h->d_roots, (const double*)(h->d_roots + DC), gx_out,
                         B, Bg, DC);
      ZF_CHECK_LAUNCH("bn_bwd_kernel");
    }
  }
  // the gradient close, as the trainer's close_gradient: every rank's fp64 share, the tree over the ranks, fp32
  if (W > 1) {
    rc = h->comm.allgather(h->comm.ctx, h->d_g64, h->d_gath, (size_t)h->nat_floats * sizeof(double), st);
    if (rc) return rc;
#define ZF_L(NM) hipLaunchKernelGGL((tree_cols_cast_kernel<NM>), dim3(blocks_for(h->nat_floats)), dim3(256), 0, st, \
                                    (const double*)h->d_gath, W, (long long)h->nat_floats, h->d_grad)
    ZF_NMAX_DISPATCH(W, ZF_L);
#undef ZF_L
    ZF_CHECK_LAUNCH("tree_cols_cast_kernel");
  } else {
    hipLaunchKernelGGL(cast_f64_f32_kernel, dim3(blocks_for(h->nat_floats)), dim3(256), 0, st,
                       (const double*)h->d_g64, (long long)h->nat_floats, h->d_grad, (float*)nullptr, 0.f, 0.f);
    ZF_CHECK_LAUNCH("cast_f64_f32_kernel");
  }
  h->have_grad = true;
  if (grad_out && grad_out != h->d_grad)
    ZF_TRY_HIP(hipMemcpyAsync(grad_out, h->d_grad, (size_t)h->nat_floats * sizeof(float), hipMemcpyDeviceToDevice, st));
  return ZF_OK;
}

// Both reverse entries: zf_condnet_backward is the view without gx_out.
int cn_backward_entry(zf_condnet* h, const float* gc, float* grad_out, float* gx_out, bool want_gx, void* stream) {
  if (!h) return einval("condnet is NULL");
  if (!h->pending) return einval("no forward pending");
  if (!gc) return einval("gc is NULL");
  if (want_gx && !gx_out) return einval("gx_out is NULL");  // the pass stays pending
  h->pending = false;  // one backward per forward
  return cn_backward(h, gc, grad_out, gx_out, (hipStream_t)stream);
}

}  // namespace
}  // namespace zf

extern "C" {

int64_t zf_segment_workspace_bytes(int64_t rows, int64_t sets, int F) {
  if (rows < 0 || sets < 0 || F < 1 || F > 64) return 0;
  return zf::seg_ws_bytes(rows, sets, F);
}

int zf_segment_sum(const float* h, int64_t rows, int F, const int64_t* off, int64_t sets, float rate, uint64_t seed,
                   float* out, int32_t* set_index, void* workspace, void* stream) {
  const int rc = zf::seg_check(h, off, out, rows, F, sets, rate);
  if (rc) return rc;
  if (!workspace) return zf::einval("segment: NULL workspace");
  return zf::seg_sum_launch(h, rows, F, (const long long*)off, sets, rate, seed, out, set_index, workspace,
                            (hipStream_t)stream);
}

int zf_segment_bcast(const float* gc, const int32_t* set_index, int64_t rows, int F, int64_t sets, float rate,
                     uint64_t seed, float* g_h, void* stream) {
  const int rc = zf::seg_check(gc, set_index, g_h, rows, F, sets, rate);
  if (rc) return rc;
  return zf::seg_bcast_launch(gc, set_index, rows, F, sets, rate, seed, 0, g_h, (hipStream_t)stream);
}

int64_t zf_segment_pool_workspace_bytes(int64_t rows, int64_t sets, int F, int pool) {
  if (rows < 0 || sets < 0 || F < 1 || F > 64 || !zf::seg_pool_known(pool)) return 0;
  return zf::seg_pool_ws_bytes(rows, sets, F, pool);
}

int zf_segment_pool(const float* h, int64_t rows, int F, const int64_t* off, int64_t sets, int pool, float rate,
                    uint64_t seed, float* out, int32_t* set_index, int32_t* count, void* workspace, void* stream) {
  if (!zf::seg_pool_known(pool)) return zf::einval("segment: unknown pool %d", pool);
  const int rc = zf::seg_check(h, off, out, rows, F, sets, rate);
  if (rc) return rc;
  if (!workspace) return zf::einval("segment: NULL workspace");
  return zf::seg_pool_launch(h, rows, F, (const long long*)off, sets, pool, rate, seed, 0, out, set_index, count,
                             workspace, (hipStream_t)stream);
}

int zf_segment_pool_bcast(const float* gc, const int32_t* set_index, int64_t rows, int F, int64_t sets, int pool,
                          float rate, uint64_t seed, const float* h, const float* out, const int32_t* count,
                          float* g_h, void* stream) {
  if (!zf::seg_pool_known(pool)) return zf::einval("segment: unknown pool %d", pool);
  const int rc = zf::seg_check(gc, set_index, g_h, rows, F, sets, rate);
  if (rc) return rc;
  if (pool != ZF_POOL_SUM && !count) return zf::einval("segment: NULL count");
  if (pool == ZF_POOL_MAX && (!h || !out)) return zf::einval("segment: the max's reverse needs h and out");
  return zf::seg_pool_bcast_launch(gc, set_index, rows, F, sets, pool, rate, seed, 0, h, out, count, g_h,
                                   (hipStream_t)stream);
}

int zf_segment_repeat(const float* c, int64_t sets, int F, const int64_t* off, int64_t rows, float* out,
                      int32_t* set_index, void* workspace, void* stream) {
  const int rc = zf::seg_check(c, off, out, rows, F, sets, 0.f);
  if (rc) return rc;
  if (!workspace) return zf::einval("segment: NULL workspace");
  return zf::seg_repeat_launch(c, sets, F, (const long long*)off, rows, out, set_index, workspace,
                               (hipStream_t)stream);
}

int zf_condnet_plan(zf_condnet_desc* d, int64_t* blob_floats) {
  if (!d || !blob_floats) return zf::einval("NULL argument");
  if (d->in_dim < 1) return zf::einval("condnet: in_dim %d", d->in_dim);
  if (d->in_dim > 64) return zf::enotsup("condnet: more than 64 input columns");
  if (d->out_dim < 1) return zf::einval("condnet: out_dim %d", d->out_dim);
  if (d->out_dim > 64) return zf::enotsup("condnet: more than 64 output columns");
  if (d->n_hidden < 0) return zf::einval("condnet: n_hidden %d", d->n_hidden);
  if (d->n_hidden > 16) return zf::enotsup("condnet: more than 16 hidden layers");
  for (int l = 0; l < d->n_hidden; ++l) {
    if (d->hidden[l] < 1) return zf::einval("condnet: hidden[%d] = %d", l, d->hidden[l]);
    if (d->hidden[l] > 4096) return zf::enotsup("condnet: a hidden width above 4096");
  }
  if (d->act < 0 || d->act >= ZF_ACT_COUNT) return zf::einval("condnet: unknown activation %d", d->act);
  // (the mean is a standalone reduction only, zf_segment_pool: a network rejects its code as it always has)
  if (d->pool != ZF_POOL_NONE && d->pool != ZF_POOL_SUM && d->pool != ZF_POOL_MAX)
    return zf::einval("condnet: unknown pool %d", d->pool);
  if (!(d->dropout >= 0.f && d->dropout < 1.f)) return zf::einval("condnet: dropout %g outside [0, 1)", (double)d->dropout);
  if (d->batch_norm != 0 && d->batch_norm != 1) return zf::einval("condnet: batch_norm %d", d->batch_norm);
  int64_t at = 0;
  auto take = [&](int64_t n) {
    const int64_t o = at;
    at += (n + 3) / 4 * 4;
    return o;
  };
  d->off_bn = d->batch_norm ? take(4ll * d->in_dim) : -1;
  for (int l = 0; l < 17; ++l) d->off_w[l] = d->off_b[l] = -1;
  int in_w = d->in_dim;
  for (int l = 0; l <= d->n_hidden; ++l) {
    const int out_w = l == d->n_hidden ? d->out_dim : d->hidden[l];
    d->off_w[l] = take((int64_t)in_w * out_w);
    d->off_b[l] = take(out_w);
    in_w = out_w;
  }
  *blob_floats = at;
  return ZF_OK;
}

int zf_condnet_create(const zf_condnet_desc* desc_in, const float* blob_host, int64_t blob_floats,
                      const unsigned char* param_mask, int64_t rows_max, int64_t sets_max,
                      const zf_optim_desc* optim, zf_condnet_t** out) {
  if (!desc_in || !blob_host || !param_mask || !out) return zf::einval("NULL argument");
  *out = nullptr;
  zf_condnet_desc desc = *desc_in;
  int64_t need = 0;
  int rc = zf_condnet_plan(&desc, &need);
  if (rc) return rc;
  if (need != blob_floats)
    return zf::einval("blob has %lld floats, plan needs %lld", (long long)blob_floats, (long long)need);
  if (rows_max < 1 || rows_max > (1 << 24)) return zf::einval("rows_max outside [1, 2^24]");
  const bool pool = desc.pool != ZF_POOL_NONE;
  if (pool && (sets_max < 1 || sets_max > zf::kSegMaxSets)) return zf::einval("sets_max outside [1, 2^24]");
  const zf_optim_desc dflt{1e-3f, 0.9f, 0.999f, 1e-8f, 1e-4f, 1};
  const zf_optim_chain chain = zf::adamw_chain(optim ? *optim : dflt);
  zf::ChainPlan plan;
  if ((rc = zf::optim_plan_chain(&chain, false, &plan))) return rc;
  zf_condnet* h = new zf_condnet();
  h->desc = desc;
  h->in = desc.in_dim;
  h->F = desc.out_dim;
  h->L = desc.n_hidden;
  h->nat_floats = need;
  h->rows_max = rows_max;
  h->sets_max = pool ? sets_max : 0;
  const int64_t B = rows_max;
  int wmax = std::max(h->in, h->F);
  for (int l = 0; l < h->L; ++l) wmax = std::max(wmax, desc.hidden[l]);
  // what an eval-mode forward touches; the reverse pass's buffers come with the first train-mode pass (cn_ensure_train)
  h->wmax = wmax;
  h->d_nat = zf::cn_alloc<float>(h, need, rc);
  h->d_mask = zf::cn_alloc<unsigned char>(h, need, rc);
  h->d_ubn = zf::cn_alloc<float>(h, B * h->in, rc);
  h->d_mean = zf::cn_alloc<float>(h, 64, rc);
  h->d_rstd = zf::cn_alloc<float>(h, 64, rc);
  for (int l = 0; l < h->L; ++l) h->H.push_back(zf::cn_alloc<float>(h, B * desc.hidden[l], rc));
  h->d_h = zf::cn_alloc<float>(h, B * h->F, rc);
  h->d_segws = zf::cn_alloc<char>(h, zf::seg_pool_ws_bytes(B, h->sets_max, h->F, desc.pool), rc);
  h->d_split = zf::cn_alloc<float>(h, zf::kSplitFloats, rc);
  hipError_t e = hipSuccess;
  if (!rc) e = hipMemcpy(h->d_nat, blob_host, need * sizeof(float), hipMemcpyHostToDevice);
  if (!rc && e == hipSuccess) e = hipMemcpy(h->d_mask, param_mask, need, hipMemcpyHostToDevice);
  if (!rc && e != hipSuccess) rc = zf::hip_status(e, "zf_condnet_create");
  if (!rc) rc = zf::cn_install_chain(h, plan, nullptr);
  if (rc) {
    zf_condnet_destroy(h);
    return rc;
  }
  *out = h;
  return ZF_OK;
}

int zf_condnet_destroy(zf_condnet_t* h) {
  if (!h) return ZF_OK;
  (void)hipDeviceSynchronize();
  for (void* p : h->bufs) (void)hipFree(p);
  zf::cn_free_chain(h);
  if (h->d_gath) (void)hipFree(h->d_gath);
  delete h;
  return ZF_OK;
}

int zf_condnet_set_comm(zf_condnet_t* h, const zf_comm_desc* comm) {
  if (!h) return zf::einval("condnet is NULL");
  zf_comm_desc c{0, 1, nullptr, nullptr};
  if (comm) c = *comm;
  if (c.world < 1 || c.rank < 0 || c.rank >= c.world) return zf::einval("bad rank %d / world %d", c.rank, c.world);
  if (c.world > zf::kMaxLeaves) return zf::enotsup("condnet: more than 64 ranks");
  if (c.world > 1 && !c.allgather) return zf::einval("communicator without allgather");
  // the gather buffer only grows (largest exchange: the fp64 gradient of every rank)
  const int64_t need =
      c.world > 1 ? std::max<int64_t>(h->nat_floats, 256) * (int64_t)sizeof(double) * c.world : 0;
  if (need > h->gath_bytes) {
    ZF_TRY_HIP(hipDeviceSynchronize());
    if (h->d_gath) (void)hipFree(h->d_gath);
    h->d_gath = nullptr;
    h->gath_bytes = 0;
    ZF_TRY_HIP(hipMalloc((void**)&h->d_gath, (size_t)need));
    h->gath_bytes = need;
  }
  h->pending = false;  // a pending pass belongs to the layout it ran under
  h->comm = c;
  return ZF_OK;
}

int zf_condnet_forward(zf_condnet_t* h, const float* x, int64_t rows, const int64_t* off, int64_t sets, int train,
                       int update_stats, uint64_t seed, float* c_out, void* stream) {
  return zf_condnet_forward_shard(h, x, rows, rows, 0, off, sets, train, update_stats, seed, c_out, stream);
}

int zf_condnet_forward_shard(zf_condnet_t* h, const float* x, int64_t rows, int64_t global_rows, int64_t row_base,
                             const int64_t* off, int64_t sets, int train, int update_stats, uint64_t seed,
                             float* c_out, void* stream) {
  if (!h) return zf::einval("condnet is NULL");
  h->pending = false;
  if (!x || !c_out) return zf::einval("NULL argument");
  if (rows < 1 || rows > h->rows_max)
    return zf::einval("rows %lld outside [1, rows_max = %lld]", (long long)rows, (long long)h->rows_max);
  if (global_rows < rows || row_base < 0 || row_base > global_rows - rows ||
      (h->comm.world == 1 && global_rows != rows))
    return zf::einval("global_rows %lld, row_base %lld vs rows %lld (world %d)", (long long)global_rows,
                      (long long)row_base, (long long)rows, h->comm.world);
  const bool pool = h->desc.pool != ZF_POOL_NONE;
  if (pool) {
    if (!off) return zf::einval("a pooled network needs the sets' offsets");
    if (sets < 1 || sets > h->sets_max)
      return zf::einval("sets %lld outside [1, sets_max = %lld]", (long long)sets, (long long)h->sets_max);
  } else if (off) {
    return zf::einval("offsets given to a network without pooling");
  }
  if (!train && update_stats) return zf::einval("update_stats needs train mode (eval mode reads the stored statistics)");
  int rc = train ? zf::cn_ensure_train(h) : ZF_OK;
  if (rc) return rc;
  rc = zf::cn_forward(h, x, (int)rows, global_rows, row_base, (const long long*)off, pool ? sets : 0, train ? 1 : 0,
                      update_stats ? 1 : 0, seed, c_out, (hipStream_t)stream);
  if (rc) return rc;
  if (train) {
    h->pending = true;
    h->pend_rows = rows;
    h->pend_global = global_rows;
    h->pend_base = row_base;
    h->pend_sets = pool ? sets : 0;
    h->pend_seed = seed;
  }
  return ZF_OK;
}

int zf_condnet_backward(zf_condnet_t* h, const float* gc, float* grad_out, void* stream) {
  return zf::cn_backward_entry(h, gc, grad_out, nullptr, false, stream);
}

int zf_condnet_backward_input(zf_condnet_t* h, const float* gc, float* grad_out, float* gx_out, void* stream) {
  return zf::cn_backward_entry(h, gc, grad_out, gx_out, true, stream);
}

int zf_condnet_apply_gradient(zf_condnet_t* h, const float* grad, void* stream) {
  if (!h) return zf::einval("condnet is NULL");
  if (!grad && !h->have_grad) return zf::einval("no gradient: apply_gradient(NULL) needs an earlier backward");
  h->pending = false;  // the parameters the activations belong to are about to change
  hipStream_t st = (hipStream_t)stream;
  const int rc = zf::cn_ensure_train(h);
  if (rc) return rc;
  if (grad && grad != h->d_grad) {
    ZF_TRY_HIP(hipMemcpyAsync(h->d_grad, grad, (size_t)h->nat_floats * sizeof(float), hipMemcpyDeviceToDevice, st));
    h->have_grad = true;
  }
  const zf::ChainPlan& p = h->plan;
  return zf::optim_chain_step(h->d_nat, h->d_grad, h->d_mask, h->d_dmask, (long long)h->nat_floats, p.args, p.form,
                              p.clip, p.max_norm, p.has_lr, p.sched, p.has_adam, p.b1, p.b2, h->d_osc, h->d_nleaf,
                              h->n_nleaf, st);
}

int zf_condnet_set_optim_chain(zf_condnet_t* h, const zf_optim_chain* chain, const unsigned char* decay_mask) {
  if (!h || !chain) return zf::einval("NULL argument");
  zf::ChainPlan plan;
  const int rc = zf::optim_plan_chain(chain, decay_mask != nullptr, &plan);
  if (rc) return rc;
  ZF_TRY_HIP(hipDeviceSynchronize());
  return zf::cn_install_chain(h, plan, decay_mask);
}

// The optimiser state, as zf_trainer_{get,set}_opt_*: a handle's optimiser is always a chain.
static int cn_opt_slot_ptr(zf_condnet_t* h, int slot, float** p) {
  if (!h) return zf::einval("condnet is NULL");
  const int n = h->plan.n_slots;
  if (slot < 0 || slot >= n) return zf::einval("optimiser slot %d outside [0, %d)", slot, n);
  *p = h->plan.args.slot[slot];
  return ZF_OK;
}

int zf_condnet_get_opt_slot(zf_condnet_t* h, int slot, float* host_floats) {
  float* p = nullptr;
  const int rc = cn_opt_slot_ptr(h, slot, &p);
  if (rc) return rc;
  if (!host_floats) return zf::einval("NULL argument");
  ZF_TRY_HIP(hipDeviceSynchronize());
  ZF_TRY_HIP(hipMemcpy(host_floats, p, h->nat_floats * sizeof(float), hipMemcpyDeviceToHost));
  return ZF_OK;
}

int zf_condnet_set_opt_slot(zf_condnet_t* h, int slot, const float* host_floats) {
  float* p = nullptr;
  const int rc = cn_opt_slot_ptr(h, slot, &p);
  if (rc) return rc;
  if (!host_floats) return zf::einval("NULL argument");
  ZF_TRY_HIP(hipDeviceSynchronize());
  ZF_TRY_HIP(hipMemcpy(p, host_floats, h->nat_floats * sizeof(float), hipMemcpyHostToDevice));
  return ZF_OK;
}

int zf_condnet_get_opt_scalars(zf_condnet_t* h, int64_t* count, double* learning_rate, double* grad_norm) {
  if (!h) return zf::einval("condnet is NULL");
  ZF_TRY_HIP(hipDeviceSynchronize());
  zf::OptScalars sc;
  ZF_TRY_HIP(hipMemcpy(&sc, h->d_osc, sizeof(sc), hipMemcpyDeviceToHost));
  if (count) *count = sc.count;
  if (learning_rate) *learning_rate = sc.count > 0 ? (double)sc.lr : (double)__builtin_nanf("");  // no step yet
  if (grad_norm) *grad_norm = sc.count > 0 ? sc.norm : (double)__builtin_nanf("");
  return ZF_OK;
}

int zf_condnet_set_opt_count(zf_condnet_t* h, int64_t count) {
  if (!h) return zf::einval("condnet is NULL");
  if (count < 0 || count > 0x7fffffff) return zf::einval("optimiser count %lld outside [0, 2^31)", (long long)count);
  ZF_TRY_HIP(hipDeviceSynchronize());
  const long long c = count;
  ZF_TRY_HIP(hipMemcpy(&h->d_osc->count, &c, sizeof(c), hipMemcpyHostToDevice));
  return ZF_OK;
}

int zf_condnet_get_blob(zf_condnet_t* h, float* blob_host) {
  if (!h || !blob_host) return zf::einval("NULL argument");
  ZF_TRY_HIP(hipDeviceSynchronize());
  ZF_TRY_HIP(hipMemcpy(blob_host, h->d_nat, h->nat_floats * sizeof(float), hipMemcpyDeviceToHost));
  return ZF_OK;
}

int zf_condnet_set_blob(zf_condnet_t* h, const float* blob_host) {
  if (!h || !blob_host) return zf::einval("NULL argument");
  h->pending = false;
  ZF_TRY_HIP(hipDeviceSynchronize());
  ZF_TRY_HIP(hipMemcpy(h->d_nat, blob_host, h->nat_floats * sizeof(float), hipMemcpyHostToDevice));
  return ZF_OK;
}

}  // extern "C"
