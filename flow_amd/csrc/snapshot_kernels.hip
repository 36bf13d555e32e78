// Reductions of a time series of fields kept in HBM (flow_amd/fem/
// snapshots.py): the two tall-and-skinny kernels behind fem.Snapshots.  X is a
// column-major store: column j starts at X + j*ldx, ldx >= n and even, X 16-byte
// aligned, so every column can be read as double2.
//
//   flow_multi_dot  out[j] = sum_i X[j*ldx + i] * y[i], j < m.  The columns are
//                   taken in chunks of kChunk = 8 (grid.y; the last chunk may
//                   hold fewer: its own instance); the 8 accumulators of a lane
//                   share one load of y.  grid.x depends on n alone: min(
//                   kRedBlocks, ceil(ceil(n/2) / kBlock)).  A lane takes the
//                   entry pairs p = block*kBlock + thread, p + grid.x*kBlock, ...
//                   in ascending order and adds (2p) then (2p + 1) to the
//                   column's accumulator by fma; a last single entry of an odd
//                   n is added alone.  The block sum has a fixed shape (shuffle
//                   tree over the 64 lanes of a wave, then wave 0 + 1 + 2 + 3);
//                   block b leaves its sums in work[b*m + j], and a finishing
//                   launch, one lane per column, adds them for b = 0, 1, ... in
//                   that order.  Nothing in the chain of one column involves
//                   another column or m: out[j] has the same bits whatever m is
//                   and wherever the column sits in its chunk, and two calls
//                   agree bit for bit.  No atomics.  (The chain itself:
//                   multi_dot.h, shared with flow_block_gram.)
//   flow_combine    out[k*ldo + i] = (base ? base[i] : 0) + sum_j C[k*m + j] *
//                   X[j*ldx + i], k < r, the terms added in ascending j by fma.
//                   One lane per row i; the outputs are taken in chunks of
//                   kChunk (grid.y), so X[j][i] is loaded once per chunk.  The
//                   coefficients of a chunk are staged through LDS in tiles of
//                   kCoefTile columns (vector loads by the first lanes of the
//                   block, read back as broadcasts): they are wave-uniform, and
//                   what a kernel reads through the scalar cache right behind
//                   the kernel that wrote it has been seen stale on this part
//                   (common.h, load_scalar).
//
// Both are plain fp64 vector FMA: bandwidth-bound at 8 (m + ceil(m/8)) n and
// 8 (m ceil(r/8) + r) n bytes.
#include <climits>
#include <cstdint>

#include "common.h"
#include "multi_dot.h"

namespace flow {
namespace {

constexpr int kCoefTile = 32;    // columns of C staged in LDS at a time
constexpr int kMaxGridY = 65535;

// columns j0 + blockIdx.y*kChunk .. + MC of X against y
template <int MC>
__global__ __launch_bounds__(kBlock) void multi_dot_kernel(
    int n, int m, int j0, const double* __restrict__ X, size_t ldx,
    const double* __restrict__ y, double* __restrict__ work) {
  const int jc = j0 + blockIdx.y * kChunk;
  dot_columns<MC>(n, X + static_cast<size_t>(jc) * ldx, ldx, y,
                  work + static_cast<size_t>(blockIdx.x) * m + jc, 1);
}

// outputs k0 + blockIdx.y*kChunk .. + RC, one lane per row
template <int RC>
__global__ __launch_bounds__(kBlock) void combine_kernel(
    int n, int m, int k0, const double* __restrict__ X, size_t ldx,
    const double* __restrict__ C, const double* __restrict__ base,
    double* __restrict__ out, size_t ldo) {
  __shared__ double coef[kCoefTile][RC];
  const int kc = k0 + blockIdx.y * kChunk;
  const int i = blockIdx.x * kBlock + threadIdx.x;
  const bool live = i < n;
  const double b = (live && base) ? base[i] : 0.0;
  double acc[RC];
#pragma unroll
  for (int k = 0; k < RC; ++k) acc[k] = b;
  for (int t0 = 0; t0 < m; t0 += kCoefTile) {
    const int nt = min(kCoefTile, m - t0);
    __syncthreads();   // the previous tile has been read
    if (threadIdx.x < kCoefTile * RC) {
      const int k = threadIdx.x / kCoefTile, t = threadIdx.x - k * kCoefTile;
      if (t < nt) coef[t][k] = C[static_cast<size_t>(kc + k) * m + t0 + t];
    }
    __syncthreads();
    if (live) {
      const double* __restrict__ x = X + static_cast<size_t>(t0) * ldx + i;
#pragma unroll 4
      for (int t = 0; t < nt; ++t) {
        const double xv = x[static_cast<size_t>(t) * ldx];
#pragma unroll
        for (int k = 0; k < RC; ++k) acc[k] = fma(coef[t][k], xv, acc[k]);
      }
    }
  }
  if (live) {
#pragma unroll
    for (int k = 0; k < RC; ++k) out[static_cast<size_t>(kc + k) * ldo + i] = acc[k];
  }
}

static_assert(kCoefTile * kChunk <= kBlock, "one lane per staged coefficient");

template <int MC>
void launch_dot(int g, int chunks, int n, int m, int j0, const double* X, size_t ldx,
                const double* y, double* work, hipStream_t st) {
  hipLaunchKernelGGL((multi_dot_kernel<MC>), dim3(g, chunks), dim3(kBlock), 0, st, n, m,
                     j0, X, ldx, y, work);
}

template <int RC>
void launch_combine(int g, int chunks, int n, int m, int k0, const double* X, size_t ldx,
                    const double* C, const double* base, double* out, size_t ldo,
                    hipStream_t st) {
  hipLaunchKernelGGL((combine_kernel<RC>), dim3(g, chunks), dim3(kBlock), 0, st, n, m, k0,
                     X, ldx, C, base, out, ldo);
}

}  // namespace
}  // namespace flow

using namespace flow;

extern "C" int flow_multi_dot(int n, int m, const double* X, size_t ldx, const double* y,
                              double* work, double* out, void* stream) {
  FLOW_REQUIRE(n >= 0 && m >= 0, "multi-dot sizes");
  if (n == 0 || m == 0) return FLOW_OK;
  FLOW_REQUIRE(X && y && work && out, "multi-dot pointers");
  FLOW_REQUIRE(ldx >= static_cast<size_t>(n) && ldx % 2 == 0, "multi-dot: ldx >= n, even");
  FLOW_REQUIRE(aligned16(X) && aligned16(y), "multi-dot: X and y 16-byte aligned");
  hipStream_t st = as_stream(stream);
  const int g = dot_grid(n);
  const int whole = m / kChunk, rest = m % kChunk;
  for (int c0 = 0; c0 < whole; c0 += kMaxGridY)
    launch_dot<kChunk>(g, std::min(kMaxGridY, whole - c0), n, m, c0 * kChunk, X, ldx, y,
                       work, st);
  const int j0 = whole * kChunk;
  switch (rest) {
    case 1: launch_dot<1>(g, 1, n, m, j0, X, ldx, y, work, st); break;
    case 2: launch_dot<2>(g, 1, n, m, j0, X, ldx, y, work, st); break;
    case 3: launch_dot<3>(g, 1, n, m, j0, X, ldx, y, work, st); break;
    case 4: launch_dot<4>(g, 1, n, m, j0, X, ldx, y, work, st); break;
    case 5: launch_dot<5>(g, 1, n, m, j0, X, ldx, y, work, st); break;
    case 6: launch_dot<6>(g, 1, n, m, j0, X, ldx, y, work, st); break;
    case 7: launch_dot<7>(g, 1, n, m, j0, X, ldx, y, work, st); break;
    default: break;
  }
  hipLaunchKernelGGL(multi_dot_finish_kernel, dim3((m + kBlock - 1) / kBlock), dim3(kBlock),
                     0, st, m, g, work, out);
  // one check behind all launches: hipGetLastError keeps the first failure
  FLOW_CHECK_LAUNCH();
  return FLOW_OK;
}

extern "C" int flow_combine(int n, int m, const double* X, size_t ldx, int r,
                            const double* C, const double* base, double* out, size_t ldo,
                            void* stream) {
  FLOW_REQUIRE(n >= 0 && m >= 1 && r >= 0, "combine sizes");
  if (n == 0 || r == 0) return FLOW_OK;
  FLOW_REQUIRE(X && C && out, "combine pointers");
  FLOW_REQUIRE(ldx >= static_cast<size_t>(n) && ldo >= static_cast<size_t>(n),
               "combine: ldx >= n, ldo >= n");
  const size_t nn = static_cast<size_t>(n);
  const size_t xspan = static_cast<size_t>(m - 1) * ldx + nn;
  const size_t ospan = static_cast<size_t>(r - 1) * ldo + nn;
  FLOW_REQUIRE(!overlap(out, ospan, X, xspan), "combine: out overlaps X");
  FLOW_REQUIRE(!base || !overlap(out, ospan, base, nn), "combine: out overlaps base");
  FLOW_REQUIRE(!overlap(out, ospan, C, static_cast<size_t>(r) * m),
               "combine: out overlaps C");
  hipStream_t st = as_stream(stream);
  const int g = (n + kBlock - 1) / kBlock;
  const int whole = r / kChunk, rest = r % kChunk;
  for (int c0 = 0; c0 < whole; c0 += kMaxGridY)
    launch_combine<kChunk>(g, std::min(kMaxGridY, whole - c0), n, m, c0 * kChunk, X, ldx,
                           C, base, out, ldo, st);
  const int k0 = whole * kChunk;
  switch (rest) {
    case 1: launch_combine<1>(g, 1, n, m, k0, X, ldx, C, base, out, ldo, st); break;
    case 2: launch_combine<2>(g, 1, n, m, k0, X, ldx, C, base, out, ldo, st); break;
    case 3: launch_combine<3>(g, 1, n, m, k0, X, ldx, C, base, out, ldo, st); break;
    case 4: launch_combine<4>(g, 1, n, m, k0, X, ldx, C, base, out, ldo, st); break;
    case 5: launch_combine<5>(g, 1, n, m, k0, X, ldx, C, base, out, ldo, st); break;
    case 6: launch_combine<6>(g, 1, n, m, k0, X, ldx, C, base, out, ldo, st); break;
    case 7: launch_combine<7>(g, 1, n, m, k0, X, ldx, C, base, out, ldo, st); break;
    default: break;
  }
  // one check behind all launches: hipGetLastError keeps the first failure
  FLOW_CHECK_LAUNCH();
  return FLOW_OK;
}
