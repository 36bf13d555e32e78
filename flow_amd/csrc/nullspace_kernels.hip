// Deflation against a small orthonormal basis kept in HBM (flow_amd/fem/
// nullspace.py): x <- x - sum_j Z_j (Z_j^T x), what the mixed Krylov loops and
// Newton's method run once per iteration to stay off a known nullspace.  Z is a
// column-major store with the conventions of flow_multi_dot: column j at
// Z + j*ldz, ldz >= n and even, Z and x 16-byte aligned.
//
//   flow_deflate   two launches, no temporary, no host wait, no atomics.
//       launch 1   multi_dot_kernel of snapshot_kernels.hip for k <= 8 columns:
//                  dot_columns<K> (multi_dot.h) -- the lane order, the block sum
//                  and the grid rule dot_grid(n) of flow_multi_dot --, block b
//                  leaving its K sums in work[b*K + j].
//       launch 2   every block first forms c_j = the block partials of column
//                  j added in ascending block order from 0.0, the sum
//                  multi_dot_finish_kernel forms: the partials (at most 1024
//                  per column) are staged through LDS in tiles of kPartTile
//                  blocks by all lanes (vector loads: what a kernel reads
//                  through the scalar cache right behind the kernel that wrote
//                  it has been seen stale on this part, common.h), lane j < K
//                  adds its column's.  c_j goes back through LDS as a
//                  broadcast; the block then takes entry pairs in a grid-stride
//                  loop, x[i] = fma(-c_j, Z_j[i], x[i]) for j ascending -- what
//                  flow_combine(base = x, C = -c) computes per entry.  Block 0
//                  writes c to coef.
//
// The chain of c_j involves n, column j and x alone; the chain of x[i] the
// c_j in ascending j: neither depends on K or on a column's place beyond that
// order, and two calls agree bit for bit.
//
// Plain fp64 vector FMA, bandwidth-bound: 8 n (2 K + 3) bytes (launch 1 reads
// Z and x, launch 2 reads both again and writes x).
#include <cstdint>

#include "common.h"
#include "multi_dot.h"

namespace flow {
namespace {

constexpr int kPartTile = 256;   // block partials of every column per LDS tile

template <int K>
__global__ __launch_bounds__(kBlock) void deflate_dot_kernel(
    int n, const double* __restrict__ Z, size_t ldz, const double* __restrict__ x,
    double* __restrict__ work) {
  dot_columns<K>(n, Z, ldz, x, work + static_cast<size_t>(blockIdx.x) * K, 1);
}

template <int K>
__global__ __launch_bounds__(kBlock) void deflate_update_kernel(
    int n, int nparts, const double* __restrict__ Z, size_t ldz, double* __restrict__ x,
    const double* __restrict__ work, double* __restrict__ coef) {
  __shared__ double part[kPartTile * K];
  __shared__ double cs[K];
  double s = 0.0;
  for (int b0 = 0; b0 < nparts; b0 += kPartTile) {
    const int nb = min(kPartTile, nparts - b0);
    __syncthreads();   // the previous tile has been read
    for (int t = threadIdx.x; t < nb * K; t += kBlock)
      part[t] = work[static_cast<size_t>(b0) * K + t];
    __syncthreads();
    if (threadIdx.x < K) {
#pragma unroll 8
      for (int b = 0; b < nb; ++b) s += part[b * K + threadIdx.x];
    }
  }
  if (threadIdx.x < K) {
    cs[threadIdx.x] = s;
    if (blockIdx.x == 0 && coef != nullptr) coef[threadIdx.x] = s;
  }
  __syncthreads();
  double nc[K];
#pragma unroll
  for (int j = 0; j < K; ++j) nc[j] = -cs[j];
  const int full = n / 2;                        // whole pairs
  const int stride = gridDim.x * kBlock;
  int p = blockIdx.x * kBlock + threadIdx.x;
  for (; p < full; p += stride) {
    double2 xx = reinterpret_cast<double2*>(x)[p];
    double2 zz[K];
#pragma unroll
    for (int j = 0; j < K; ++j)
      zz[j] = reinterpret_cast<const double2*>(Z + static_cast<size_t>(j) * ldz)[p];
#pragma unroll
    for (int j = 0; j < K; ++j) {
      xx.x = fma(nc[j], zz[j].x, xx.x);
      xx.y = fma(nc[j], zz[j].y, xx.y);
    }
    reinterpret_cast<double2*>(x)[p] = xx;
  }
  // the last entry of an odd n: the lane whose turn pair `full` would be
  if ((n & 1) && p == full) {
    double xl = x[n - 1];
#pragma unroll
    for (int j = 0; j < K; ++j) xl = fma(nc[j], Z[static_cast<size_t>(j) * ldz + n - 1], xl);
    x[n - 1] = xl;
  }
}

static_assert(kPartTile * kChunk * sizeof(double) <= 32768, "the LDS tile of partials");

template <int K>
void launch_deflate(int g, int g2, int n, const double* Z, size_t ldz, double* x,
                    double* work, double* coef, hipStream_t st) {
  hipLaunchKernelGGL((deflate_dot_kernel<K>), dim3(g), dim3(kBlock), 0, st, n, Z, ldz, x,
                     work);
  hipLaunchKernelGGL((deflate_update_kernel<K>), dim3(g2), dim3(kBlock), 0, st, n, g, Z,
                     ldz, x, work, coef);
}

}  // namespace
}  // namespace flow

using namespace flow;

extern "C" int flow_deflate(int n, int k, const double* Z, size_t ldz, double* x,
                            double* work, double* coef, void* stream) {
  FLOW_REQUIRE(n >= 0 && k >= 0 && k <= kChunk, "deflate sizes (k <= 8)");
  if (n == 0 || k == 0) return FLOW_OK;
  FLOW_REQUIRE(Z && x && work, "deflate pointers");
  FLOW_REQUIRE(ldz >= static_cast<size_t>(n) && ldz % 2 == 0, "deflate: ldz >= n, even");
  FLOW_REQUIRE(aligned16(Z) && aligned16(x), "deflate: Z and x 16-byte aligned");
  const size_t nn = static_cast<size_t>(n), kk = static_cast<size_t>(k);
  const size_t zspan = (kk - 1) * ldz + nn;
  const size_t wspan = kk * FLOW_MULTI_DOT_BLOCKS;
  FLOW_REQUIRE(!overlap(x, nn, Z, zspan), "deflate: x overlaps Z");
  FLOW_REQUIRE(!overlap(work, wspan, Z, zspan), "deflate: work overlaps Z");
  FLOW_REQUIRE(!overlap(work, wspan, x, nn), "deflate: work overlaps x");
  if (coef) {
    FLOW_REQUIRE(!overlap(coef, kk, Z, zspan), "deflate: coef overlaps Z");
    FLOW_REQUIRE(!overlap(coef, kk, x, nn), "deflate: coef overlaps x");
    FLOW_REQUIRE(!overlap(coef, kk, work, wspan), "deflate: coef overlaps work");
  }
  hipStream_t st = as_stream(stream);
  const int g = dot_grid(n);
  const int g2 = grid_for((static_cast<long long>(n) + 1) / 2, kBlock, kMaxGrid);
  switch (k) {
    case 1: launch_deflate<1>(g, g2, n, Z, ldz, x, work, coef, st); break;
    case 2: launch_deflate<2>(g, g2, n, Z, ldz, x, work, coef, st); break;
    case 3: launch_deflate<3>(g, g2, n, Z, ldz, x, work, coef, st); break;
    case 4: launch_deflate<4>(g, g2, n, Z, ldz, x, work, coef, st); break;
    case 5: launch_deflate<5>(g, g2, n, Z, ldz, x, work, coef, st); break;
    case 6: launch_deflate<6>(g, g2, n, Z, ldz, x, work, coef, st); break;
    case 7: launch_deflate<7>(g, g2, n, Z, ldz, x, work, coef, st); break;
    default: launch_deflate<8>(g, g2, n, Z, ldz, x, work, coef, st); break;
  }
  // one check behind both launches: hipGetLastError keeps the first failure
  FLOW_CHECK_LAUNCH();
  return FLOW_OK;
}
