// The chain of one flow_multi_dot entry (snapshot_kernels.hip), shared with
// flow_block_gram (eigen_kernels.hip): the per-lane order, the block sum and the
// finishing launch.  What both promise -- an entry depends on n and its two
// columns alone -- holds because both run THIS code.  gfx950 only.
#pragma once
#include <cstdint>

#include "common.h"

namespace flow {
namespace {

constexpr int kChunk = 8;        // columns (outputs) a lane keeps in registers

// grid.x of flow_multi_dot: a function of n alone
inline int dot_grid(int n) {
  const long long pairs = (static_cast<long long>(n) + 1) / 2;
  return grid_for(pairs, kBlock, kRedBlocks);
}

// The share of workgroup blockIdx.x (of gridDim.x) in the dot products of the
// MC columns X0, X0 + ldx, ... against y: column c's into out[c * ostride].
template <int MC>
__device__ __forceinline__ void dot_columns(
    int n, const double* __restrict__ X0, size_t ldx, const double* __restrict__ y,
    double* __restrict__ out, size_t ostride) {
  __shared__ double wave_part[MC][4];
  const double* __restrict__ col[MC];
#pragma unroll
  for (int c = 0; c < MC; ++c) col[c] = X0 + static_cast<size_t>(c) * ldx;
  double acc[MC];
#pragma unroll
  for (int c = 0; c < MC; ++c) acc[c] = 0.0;
  const int full = n / 2;                        // whole pairs
  const int stride = gridDim.x * kBlock;
  int p = blockIdx.x * kBlock + threadIdx.x;
  for (; p < full; p += stride) {
    const double2 yy = reinterpret_cast<const double2*>(y)[p];
    double2 xx[MC];
#pragma unroll
    for (int c = 0; c < MC; ++c) xx[c] = reinterpret_cast<const double2*>(col[c])[p];
#pragma unroll
    for (int c = 0; c < MC; ++c) {
      acc[c] = fma(xx[c].x, yy.x, acc[c]);
      acc[c] = fma(xx[c].y, yy.y, acc[c]);
    }
  }
  // the last entry of an odd n: the lane whose turn pair `full` would be
  if ((n & 1) && p == full) {
    const double yl = y[n - 1];
#pragma unroll
    for (int c = 0; c < MC; ++c) acc[c] = fma(col[c][n - 1], yl, acc[c]);
  }
#pragma unroll
  for (int c = 0; c < MC; ++c) {
    double v = acc[c];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if ((threadIdx.x & 63) == 0) wave_part[c][threadIdx.x >> 6] = v;
  }
  __syncthreads();
  if (threadIdx.x < MC) {
    const int c = threadIdx.x;
    out[static_cast<size_t>(c) * ostride] =
        wave_part[c][0] + wave_part[c][1] + wave_part[c][2] + wave_part[c][3];
  }
}

// one lane per column: the block partials in ascending block order
__global__ __launch_bounds__(kBlock) void multi_dot_finish_kernel(
    int m, int nparts, const double* __restrict__ work, double* __restrict__ out) {
  const int j = blockIdx.x * kBlock + threadIdx.x;
  if (j >= m) return;
  double s = 0.0;
#pragma unroll 8
  for (int b = 0; b < nparts; ++b) s += work[static_cast<size_t>(b) * m + j];
  out[j] = s;
}

// wave_part[..][4] and w0 + w1 + w2 + w3 in dot_columns
static_assert(kBlock == 4 * 64, "the block sum is written for four waves of 64");

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// do [a, a + na) and [b, b + nb) (in doubles) share an entry?
inline bool overlap(const double* a, size_t na, const double* b, size_t nb) {
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
  return a0 < b0 + 8 * nb && b0 < a0 + 8 * na;
}

}  // namespace
}  // namespace flow
