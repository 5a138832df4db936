// The 128 x 128 x 32 tile geometry and tile order of the persistent
// split-MFMA GEMMs (gemm_x3_kernel, zf_gemm.h; gemm_h2_kernel, zf_layered.hip)
// and the sigmoid of their epilogues.  Constants and inline device functions
// only, so any unit may include it.
#pragma once
#include <hip/hip_runtime.h>

namespace zf {
namespace {

constexpr int kX3BM = 128, kX3BN = 128, kX3BK = 32;
constexpr int kX3RS = 40;  // 16-bit elements per LDS row (32 k + 8 pad = 80 B)

__device__ __forceinline__ float sigmoidf(float z) { return 1.0f / (1.0f + expf(-z)); }

// The output tile of a persistent block's ti-th round.  Blocks go to the 8
// XCDs round-robin (block b -> XCD b % 8), each XCD with its own L2; when
// every round is full (gridDim % 8 == 0, ntiles % gridDim == 0) a round's
// tiles are dealt in runs of gridDim / 8 consecutive tiles per XCD, so the
// N-tiles of one row band (the same A rows) share an L2 instead of fetching
// the rows once per XCD.  Which block computes a tile changes nothing else.
__device__ __forceinline__ int x3_tile(int ti, int ntiles) {
  const int b = blockIdx.x, G = gridDim.x;
  if ((G & 7) == 0 && ntiles % G == 0) return ti * G + (b & 7) * (G >> 3) + (b >> 3);
  return b + ti * G;
}

}  // namespace
}  // namespace zf
