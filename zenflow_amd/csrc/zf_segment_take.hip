// Take whole sets by index (zf_segment_take, include/zenflow_amd.h): the
// element rows of take_n of S ragged sets packed contiguously, their CSR
// offsets rebuilt — a minibatch of a deep-set data set that stays resident
// on the device (zenflow_amd.train.train_sets).  Two launches:
//   take_plan_kernel    one block: the clamped offsets o (the rule of
//                       zf_segment_sum), then the scan of the taken lengths
//                       into off_out;
//   take_gather_kernel  one block per kTakeRows output rows: a bisection over
//                       off_out per row, then the copy in element order.
// Both are shaped as seg_plan_kernel / seg_repeat_kernel of zf_condnet.hip.
#include "zf_internal.h"

namespace zf {
namespace {

constexpr int64_t kTakeMaxSets = 1ll << 24;
constexpr int64_t kTakeMaxRows = (1ll << 31) - 1;  // a source row is an int32 in LDS; the grid stays below 2^31
constexpr int kPlanThreads = 1024;
constexpr int kTakeRows = 256;

// ---- the plan: one block over the S + 1 offsets, then over the take_n indices ----
// o[s] = max over j <= s of clamp(off[j], 0, rows) (off NULL: not formed, every
// set is one row).  len_t = o[take[t] + 1] - o[take[t]], 0 for an index outside
// [0, S); off_out[t + 1] = min(len_0 + ... + len_t, rows_out), which is the
// header's recurrence since no length is negative (the sum stays below 2^55).
// Thread t owns a slice of the offsets, then of the indices; the slices'
// maxima / sums are scanned through LDS (Hillis-Steele, 10 steps).
__global__ __launch_bounds__(kPlanThreads) void take_plan_kernel(const long long* __restrict__ off, long long S,
                                                                 long long rows, const long long* __restrict__ take,
                                                                 long long n, long long rows_out,
                                                                 long long* __restrict__ o,
                                                                 long long* __restrict__ off_out) {
  __shared__ long long sc[2][kPlanThreads];
  const int t = threadIdx.x;
  int cur = 0;
  if (off) {  // (uniform)
    const long long m1 = S + 1, per = (m1 + kPlanThreads - 1) / kPlanThreads;
    const long long i0 = min(m1, (long long)t * per), i1 = min(m1, i0 + per);
    long long m = 0;
    for (long long i = i0; i < i1; ++i) m = max(m, min(max(off[i], 0ll), rows));
    sc[0][t] = m;
    __syncthreads();
    for (int d = 1; d < kPlanThreads; d *= 2) {
      sc[cur ^ 1][t] = t >= d ? max(sc[cur][t], sc[cur][t - d]) : sc[cur][t];
      cur ^= 1;
      __syncthreads();
    }
    long long run = t > 0 ? sc[cur][t - 1] : 0;
    for (long long i = i0; i < i1; ++i) {
      run = max(run, min(max(off[i], 0ll), rows));
      o[i] = run;
    }
    __syncthreads();  // o[] of the whole block is visible, and sc is free again
  }
  auto len_of = [&](long long s) -> long long {
    if (s < 0 || s >= S) return 0;
    return off ? o[s + 1] - o[s] : 1;
  };
  const long long per = (n + kPlanThreads - 1) / kPlanThreads;
  const long long i0 = min(n, (long long)t * per), i1 = min(n, i0 + per);
  long long cnt = 0;
  for (long long i = i0; i < i1; ++i) cnt += len_of(take[i]);
  cur = 0;
  sc[0][t] = cnt;
  __syncthreads();
  for (int d = 1; d < kPlanThreads; d *= 2) {
    sc[cur ^ 1][t] = t >= d ? sc[cur][t] + sc[cur][t - d] : sc[cur][t];
    cur ^= 1;
    __syncthreads();
  }
  long long base = t > 0 ? sc[cur][t - 1] : 0;
  if (t == 0) off_out[0] = 0;
  for (long long i = i0; i < i1; ++i) {
    base += len_of(take[i]);
    off_out[i + 1] = min(base, rows_out);
  }
}

// ---- the gather: out[i, :] = x[source(i), :] ----------------------------------------
// One block per kTakeRows consecutive output rows.  Thread r finds the
// position t of the block's row r by bisection over off_out[0 .. n] (the last
// t with off_out[t] <= i, so empty positions are passed over; a row from
// off_out[n] on is padding: -1) and leaves the source row
// o[take[t]] + i - off_out[t] in LDS; the block then copies its kTakeRows * F
// floats in element order: consecutive lanes store consecutive floats, and
// read consecutive floats wherever their rows belong to one set.  The loads
// go to clamped addresses and the padding mask is applied at the store, four
// elements in flight per thread.  The work of a row does not depend on its
// set's length.  The launcher guarantees rows, S, n, rows_out >= 1.
__global__ __launch_bounds__(kTakeRows) void take_gather_kernel(const float* __restrict__ x, long long rows, int F,
                                                                const long long* __restrict__ o,
                                                                const long long* __restrict__ take, long long n,
                                                                const long long* __restrict__ off_out,
                                                                long long rows_out, float* __restrict__ out) {
  __shared__ int src[kTakeRows];
  const int t = threadIdx.x;
  const long long r0 = (long long)blockIdx.x * kTakeRows, i = r0 + t;
  int q = -1;
  if (i < off_out[n]) {  // (off_out[n] <= rows_out)
    long long lo = 0, hi = n;  // off_out[lo] <= i < off_out[hi]
    while (hi - lo > 1) {
      const long long mid = lo + (hi - lo) / 2;
      if (off_out[mid] <= i) lo = mid;
      else hi = mid;
    }
    // position lo is not empty, so its index is inside [0, S) and the row inside its set; the clamp is a guard
    const long long s = take[lo];
    const long long row = (o ? o[s] : s) + (i - off_out[lo]);
    q = (int)min(max(row, 0ll), rows - 1);
  }
  src[t] = q;
  __syncthreads();
  const int cnt = (int)min((long long)kTakeRows, rows_out - r0) * F;
  float* const dst = out + r0 * F;
  const int dr = kTakeRows / F, df = kTakeRows - dr * F;  // one stride of kTakeRows elements, as (rows, columns)
  int r = t / F, f = t - r * F;
  for (int e = t; e < cnt; e += 4 * kTakeRows) {
    int qs[4];
    float v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      qs[u] = src[min(r, kTakeRows - 1)];
      v[u] = x[(long long)max(qs[u], 0) * F + f];
      r += dr;
      f += df;
      if (f >= F) {
        f -= F;
        ++r;
      }
    }
    if (e + 3 * kTakeRows < cnt) {
#pragma unroll
      for (int u = 0; u < 4; ++u) dst[e + u * kTakeRows] = qs[u] >= 0 ? v[u] : 0.f;
    } else {
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (e + u * kTakeRows < cnt) dst[e + u * kTakeRows] = qs[u] >= 0 ? v[u] : 0.f;
    }
  }
}

inline long long take_ws_bytes(long long S) { return (S + 1) * (long long)sizeof(long long); }

int take_launch(const float* x, long long rows, int F, const long long* off, long long S, const long long* take,
                long long n, long long rows_out, float* out, long long* off_out, void* ws, hipStream_t st) {
  if (rows == 0 || S == 0 || n == 0 || rows_out == 0) {  // nothing can be taken: zeros, and offsets of zeros
    if (rows_out > 0) ZF_TRY_HIP(hipMemsetAsync(out, 0, (size_t)rows_out * F * sizeof(float), st));
    ZF_TRY_HIP(hipMemsetAsync(off_out, 0, (size_t)(n + 1) * sizeof(long long), st));
    return ZF_OK;
  }
  long long* o = off ? (long long*)ws : nullptr;
  hipLaunchKernelGGL(take_plan_kernel, dim3(1), dim3(kPlanThreads), 0, st, off, S, rows, take, n, rows_out, o,
                     off_out);
  ZF_CHECK_LAUNCH("take_plan_kernel");
  hipLaunchKernelGGL(take_gather_kernel, dim3((unsigned)((rows_out + kTakeRows - 1) / kTakeRows)), dim3(kTakeRows), 0,
                     st, x, rows, F, (const long long*)o, take, n, (const long long*)off_out, rows_out, out);
  ZF_CHECK_LAUNCH("take_gather_kernel");
  return ZF_OK;
}

}  // namespace
}  // namespace zf

extern "C" {

int64_t zf_segment_take_workspace_bytes(int64_t sets, int64_t take_n) {
  if (sets < 0 || take_n < 0 || sets > zf::kTakeMaxSets || take_n > zf::kTakeMaxSets) return 0;
  return zf::take_ws_bytes(sets);
}

int zf_segment_take(const float* x, int64_t rows, int F, const int64_t* off, int64_t sets, const int64_t* take,
                    int64_t take_n, int64_t rows_out, float* out, int64_t* off_out, void* workspace, void* stream) {
  if (!x || !take || !out || !off_out || !workspace) return zf::einval("segment take: NULL argument");
  if (rows < 0 || sets < 0 || take_n < 0 || rows_out < 0)
    return zf::einval("segment take: rows %lld, sets %lld, take_n %lld, rows_out %lld", (long long)rows,
                      (long long)sets, (long long)take_n, (long long)rows_out);
  if (F < 1 || F > 64) return zf::einval("segment take: F %d outside 1 .. 64", F);
  if (!off && sets != rows)
    return zf::einval("segment take: off is NULL (every set one row) with sets %lld != rows %lld", (long long)sets,
                      (long long)rows);
  if (sets > zf::kTakeMaxSets || take_n > zf::kTakeMaxSets) return zf::enotsup("segment take: more than 2^24 sets");
  if (rows > zf::kTakeMaxRows || rows_out > zf::kTakeMaxRows)
    return zf::enotsup("segment take: more than 2^31 - 1 rows");
  return zf::take_launch(x, rows, F, (const long long*)off, sets, (const long long*)take, take_n, rows_out, out,
                         (long long*)off_out, workspace, (hipStream_t)stream);
}

}  // extern "C"
