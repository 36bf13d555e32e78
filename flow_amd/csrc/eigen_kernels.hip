// The two block kernels behind fem.Eigenmodes (flow_amd/fem/eigen.py): a block
// method for A x = lambda M x spends its time multiplying one sparse matrix by a
// block of vectors and forming the Gram matrix of two blocks.  X and Y are
// column-major stores as in snapshot_kernels.hip: column j at X + j*ldx, ldx >= n
// and even, the store 16-byte aligned, the padding never read or written.
//
//   flow_operator_apply_block   Y[:, j] = A X[:, j], j < m, A of kind 0, on the
//                   CSR-stream tiles of csr_stream.h.  A workgroup loads its
//                   tile's value pairs and column pairs ONCE (StreamTile::load)
//                   and then takes the columns in chunks of MC: the gathers of
//                   all MC columns in flight together, the products parked in
//                   MC planes of LDS (MC * kTile doubles), one barrier, one
//                   row sum per lane and column, one barrier before the next
//                   chunk overwrites the planes.  The last chunk may hold fewer
//                   columns: its own instance.  The steps of a column are the
//                   steps of stream_rows_sum (the same code: gather, park, sum),
//                   so column j has the bits flow_operator_apply gives for it.
//                   Traffic: 12 B per nonzero once instead of m times; the
//                   gathers and the 8 n m B of Y are unchanged.
//                   A of kind 2 (2x2 blocks over the scalar pattern, columns of
//                   2 N entries, component-blocked): the same scheme on the
//                   rowblocks2 tiles with StreamTile2 (csr_stream.h).  The
//                   column pairs and the four planes' value pairs are loaded
//                   once (36 B per nonzero once instead of m times); per chunk
//                   the gathers of x[c], x[N + c] of all MC columns in flight,
//                   the two products per nonzero parked in two LDS planes per
//                   column (2 MC kTile2 doubles: 16 KB per column, so MC is 2
//                   or 4), one barrier, both row sums per lane and column, one
//                   barrier.  The expressions and the summation order are those
//                   of spmv_stream_block2_kernel (la_kernels.hip), so column j
//                   has the bits flow_operator_apply gives for it.
//   flow_block_gram out[i*mb + j] = X[:, i] . Y[:, j]: ONE launch over (blocks
//                   of n, chunks of 8 columns of X, columns of Y) that leaves
//                   the block sums in work[b*ma*mb + i*mb + j], and the finishing
//                   launch of flow_multi_dot over all ma*mb entries.  The chain
//                   of an entry is that of flow_multi_dot(n, ma, X, ldx, Y + j*
//                   ldy) (multi_dot.h: the same code), so it has the same bits,
//                   depends on n and its two columns alone, and two calls agree.
//                   No atomics.
#include <climits>

#include "csr_stream.h"
#include "multi_dot.h"

namespace flow {
namespace {

constexpr int kBlockMC = 2;     // columns per chunk of flow_operator_apply_block
                                // (the fastest of 2, 4, 8 at every m: 16 KB of
                                // LDS keeps 8 workgroups per CU; DESIGN.md,
                                // fem.Eigenmodes)
constexpr int kBlockMC2 = 2;    // the same for a 2x2-block operator (the faster of
                                // 2, 4 at every m: 32 KB of LDS and 94 VGPRs
                                // against 64 KB and 132; DESIGN.md,
                                // fem.Eigenmodes, tools/eigen_lab.py --vector)
constexpr int kMaxGridYZ = 65535;

// columns j .. j + C of one tile: prod holds C planes of kTile doubles
template <int C>
__device__ __forceinline__ void block_chunk(
    const StreamTile& t, const int* __restrict__ cols, int r, int r1, int j,
    const double* __restrict__ X, size_t ldx, double* __restrict__ Y, size_t ldy,
    double* __restrict__ prod) {
  StreamTile::Gathered g[C];
#pragma unroll
  for (int c = 0; c < C; ++c)      // every column's gathers before any use
    g[c] = t.gather(cols, X + static_cast<size_t>(j + c) * ldx);
#pragma unroll
  for (int c = 0; c < C; ++c) t.park(g[c], prod + c * kTile);
  __syncthreads();
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const double s = t.sum(prod + c * kTile);
    if (r < r1) Y[static_cast<size_t>(j + c) * ldy + r] = s;
  }
}

template <int MC>
__global__ __launch_bounds__(kBlock) void spmv_block_kernel(
    const int* __restrict__ rowptr, const int* __restrict__ cols,
    const double* __restrict__ vals, const int* __restrict__ rowblocks, int m,
    const double* __restrict__ X, size_t ldx, double* __restrict__ Y, size_t ldy) {
  __shared__ double prod[MC * kTile];
  const int tile = xcd_tile(blockIdx.x, gridDim.x);
  const int r0 = rowblocks[tile];
  const int r1 = rowblocks[tile + 1];
  const int r = r0 + threadIdx.x;
  StreamTile t;
  t.load(r0, r1, rowptr, cols, vals);
  int j = 0;
  for (; j + MC <= m; j += MC) {
    block_chunk<MC>(t, cols, r, r1, j, X, ldx, Y, ldy, prod);
    __syncthreads();   // the planes have been summed
  }
  // the last chunk holds fewer columns: its own instance (block-uniform)
  switch (m - j) {
    case 1: block_chunk<1>(t, cols, r, r1, j, X, ldx, Y, ldy, prod); break;
    case 2: if (MC > 2) block_chunk<2>(t, cols, r, r1, j, X, ldx, Y, ldy, prod); break;
    case 3: if (MC > 3) block_chunk<3>(t, cols, r, r1, j, X, ldx, Y, ldy, prod); break;
    case 4: if (MC > 4) block_chunk<4>(t, cols, r, r1, j, X, ldx, Y, ldy, prod); break;
    case 5: if (MC > 5) block_chunk<5>(t, cols, r, r1, j, X, ldx, Y, ldy, prod); break;
    case 6: if (MC > 6) block_chunk<6>(t, cols, r, r1, j, X, ldx, Y, ldy, prod); break;
    case 7: if (MC > 7) block_chunk<7>(t, cols, r, r1, j, X, ldx, Y, ldy, prod); break;
    default: break;
  }
}
static_assert(8 * kTile * sizeof(double) <= 65536, "LDS planes of the widest chunk");

// columns j .. j + C of one tile of a 2x2-block operator: prod holds 2 C planes
// of kTile2 doubles (column c: planes 2c and 2c + 1, the two components' products)
template <int C>
__device__ __forceinline__ void block2_chunk(
    const StreamTile2& t, int n, int r, int r1, int j, const double* __restrict__ X,
    size_t ldx, double* __restrict__ Y, size_t ldy, double* __restrict__ prod) {
  StreamTile2::Gathered g[C];
#pragma unroll
  for (int c = 0; c < C; ++c)      // every column's gathers before any use
    g[c] = t.gather(X + static_cast<size_t>(j + c) * ldx, n);
#pragma unroll
  for (int c = 0; c < C; ++c)
    t.park(g[c], prod + 2 * c * kTile2, prod + (2 * c + 1) * kTile2);
  __syncthreads();
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const double2 s = t.sum(prod + 2 * c * kTile2, prod + (2 * c + 1) * kTile2);
    if (r < r1) {
      double* __restrict__ y = Y + static_cast<size_t>(j + c) * ldy;
      y[r] = s.x;
      y[n + r] = s.y;
    }
  }
}

// full 2x2 blocks over one scalar pattern (kind 2): n rows of the pattern,
// columns of X and Y of 2 n entries, component-blocked
template <int MC>
__global__ __launch_bounds__(kBlock) void spmv_block2_kernel(
    int n, const int* __restrict__ rowptr, const int* __restrict__ cols,
    const double* __restrict__ vxx, const double* __restrict__ vxy,
    const double* __restrict__ vyx, const double* __restrict__ vyy,
    const int* __restrict__ rowblocks, int m, const double* __restrict__ X,
    size_t ldx, double* __restrict__ Y, size_t ldy) {
  __shared__ double prod[2 * MC * kTile2];
  const int tile = xcd_tile(blockIdx.x, gridDim.x);
  const int r0 = rowblocks[tile];
  const int r1 = rowblocks[tile + 1];
  const int r = r0 + threadIdx.x;
  StreamTile2 t;
  t.load(r0, r1, rowptr, cols, vxx, vxy, vyx, vyy);
  int j = 0;
  for (; j + MC <= m; j += MC) {
    block2_chunk<MC>(t, n, r, r1, j, X, ldx, Y, ldy, prod);
    __syncthreads();   // the planes have been summed
  }
  // the last chunk holds fewer columns: its own instance (block-uniform)
  switch (m - j) {
    case 1: block2_chunk<1>(t, n, r, r1, j, X, ldx, Y, ldy, prod); break;
    case 2: if (MC > 2) block2_chunk<2>(t, n, r, r1, j, X, ldx, Y, ldy, prod); break;
    case 3: if (MC > 3) block2_chunk<3>(t, n, r, r1, j, X, ldx, Y, ldy, prod); break;
    default: break;
  }
}
static_assert(2 * 4 * kTile2 * sizeof(double) <= 65536,
              "LDS planes of the widest chunk of a 2x2-block operator");

// columns blockIdx.y*kChunk .. of X against column blockIdx.z of Y
__global__ __launch_bounds__(kBlock) void block_gram_kernel(
    int n, int ma, const double* __restrict__ X, size_t ldx, int mb,
    const double* __restrict__ Y, size_t ldy, double* __restrict__ work) {
  const int ic = blockIdx.y * kChunk;
  const int jb = blockIdx.z;
  const double* __restrict__ x0 = X + static_cast<size_t>(ic) * ldx;
  const double* __restrict__ y = Y + static_cast<size_t>(jb) * ldy;
  double* __restrict__ out =
      work + (static_cast<size_t>(blockIdx.x) * ma + ic) * mb + jb;
  // the last chunk holds fewer columns: its own instance (block-uniform)
  switch (min(kChunk, ma - ic)) {
    case 1: dot_columns<1>(n, x0, ldx, y, out, mb); break;
    case 2: dot_columns<2>(n, x0, ldx, y, out, mb); break;
    case 3: dot_columns<3>(n, x0, ldx, y, out, mb); break;
    case 4: dot_columns<4>(n, x0, ldx, y, out, mb); break;
    case 5: dot_columns<5>(n, x0, ldx, y, out, mb); break;
    case 6: dot_columns<6>(n, x0, ldx, y, out, mb); break;
    case 7: dot_columns<7>(n, x0, ldx, y, out, mb); break;
    default: dot_columns<kChunk>(n, x0, ldx, y, out, mb); break;
  }
}
static_assert(kChunk == 8, "the instances of block_gram_kernel");

template <int MC>
void launch_block(const flow_operator* A, int m, const double* X, size_t ldx, double* Y,
                  size_t ldy, hipStream_t st) {
  hipLaunchKernelGGL((spmv_block_kernel<MC>), dim3(A->nblocks), dim3(kBlock), 0, st,
                     A->rowptr, A->cols, A->vals[0], A->rowblocks, m, X, ldx, Y, ldy);
}

template <int MC>
void launch_block2(const flow_operator* A, int m, const double* X, size_t ldx,
                   double* Y, size_t ldy, hipStream_t st) {
  hipLaunchKernelGGL((spmv_block2_kernel<MC>), dim3(A->nblocks), dim3(kBlock), 0, st,
                     A->n, A->rowptr, A->cols, A->vals[0], A->vals[1], A->vals[2],
                     A->vals[3], A->rowblocks, m, X, ldx, Y, ldy);
}

}  // namespace
}  // namespace flow

using namespace flow;

extern "C" int flow_operator_apply_block_chunk(const flow_operator* A, int m,
                                               const double* X, size_t ldx, double* Y,
                                               size_t ldy, int mc, void* stream) {
  int rc = check_operator(A);
  if (rc) return rc;
  FLOW_REQUIRE(A->kind == 0 || A->kind == 2,
               "block product: a scalar or a 2x2-block operator (kind 0 or 2)");
  const bool block2 = A->kind == 2;
  FLOW_REQUIRE(m >= 0, "block product: m");
  FLOW_REQUIRE(mc == 0 || mc == 2 || mc == 4 || (mc == 8 && !block2),
               "block product: chunk (2, 4; 8 for a scalar operator only)");
  if (m == 0) return FLOW_OK;
  FLOW_REQUIRE(X && Y, "block product pointers");
  const size_t n = static_cast<size_t>(A->n) * (block2 ? 2 : 1);
  FLOW_REQUIRE(ldx >= n && ldx % 2 == 0 && ldy >= n && ldy % 2 == 0,
               "block product: ldx, ldy >= n, even");
  FLOW_REQUIRE(aligned16(X) && aligned16(Y), "block product: X and Y 16-byte aligned");
  FLOW_REQUIRE(!overlap(Y, static_cast<size_t>(m - 1) * ldy + n, X,
                        static_cast<size_t>(m - 1) * ldx + n),
               "block product: Y overlaps X");
  hipStream_t st = as_stream(stream);
  if (block2) {
    if ((mc ? mc : kBlockMC2) == 2)
      launch_block2<2>(A, m, X, ldx, Y, ldy, st);
    else
      launch_block2<4>(A, m, X, ldx, Y, ldy, st);
    FLOW_CHECK_LAUNCH();
    return FLOW_OK;
  }
  switch (mc ? mc : kBlockMC) {
    case 2: launch_block<2>(A, m, X, ldx, Y, ldy, st); break;
    case 4: launch_block<4>(A, m, X, ldx, Y, ldy, st); break;
    default: launch_block<8>(A, m, X, ldx, Y, ldy, st); break;
  }
  FLOW_CHECK_LAUNCH();
  return FLOW_OK;
}

extern "C" int flow_operator_apply_block(const flow_operator* A, int m, const double* X,
                                         size_t ldx, double* Y, size_t ldy,
                                         void* stream) {
  return flow_operator_apply_block_chunk(A, m, X, ldx, Y, ldy, 0, stream);
}

extern "C" int flow_block_gram(int n, int ma, const double* X, size_t ldx, int mb,
                               const double* Y, size_t ldy, double* work, double* out,
                               void* stream) {
  FLOW_REQUIRE(n >= 0 && ma >= 0 && mb >= 0, "block gram sizes");
  if (n == 0 || ma == 0 || mb == 0) return FLOW_OK;
  FLOW_REQUIRE(X && Y && work && out, "block gram pointers");
  const size_t nn = static_cast<size_t>(n);
  FLOW_REQUIRE(ldx >= nn && ldx % 2 == 0 && ldy >= nn && ldy % 2 == 0,
               "block gram: ldx, ldy >= n, even");
  FLOW_REQUIRE(aligned16(X) && aligned16(Y), "block gram: X and Y 16-byte aligned");
  const int chunks = (ma + kChunk - 1) / kChunk;
  FLOW_REQUIRE(chunks <= kMaxGridYZ && mb <= kMaxGridYZ &&
                   static_cast<long long>(ma) * mb <= INT_MAX,
               "block gram: too many columns");
  const int g = dot_grid(n);
  const size_t entries = static_cast<size_t>(ma) * mb;
  const size_t xspan = static_cast<size_t>(ma - 1) * ldx + nn;
  const size_t yspan = static_cast<size_t>(mb - 1) * ldy + nn;
  const size_t wspan = entries * g;
  FLOW_REQUIRE(!overlap(work, wspan, X, xspan) && !overlap(work, wspan, Y, yspan) &&
                   !overlap(out, entries, X, xspan) && !overlap(out, entries, Y, yspan) &&
                   !overlap(out, entries, work, wspan),
               "block gram: work / out overlap the operands");
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(block_gram_kernel, dim3(g, chunks, mb), dim3(kBlock), 0, st, n, ma,
                     X, ldx, mb, Y, ldy, work);
  const int me = static_cast<int>(entries);
  hipLaunchKernelGGL(multi_dot_finish_kernel, dim3((me + kBlock - 1) / kBlock),
                     dim3(kBlock), 0, st, me, g, work, out);
  FLOW_CHECK_LAUNCH();
  return FLOW_OK;
}
