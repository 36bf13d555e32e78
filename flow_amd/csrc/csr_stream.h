// CSR-stream tiles of the fp64 SpMV kernels (la_kernels.hip), of the multigrid
// level kernels (krylov_kernels.hip) and of the kernels
// that carry a product with an epilogue of their own (mass_kernels.hip): a
// 256-thread workgroup owns <= 256 consecutive rows holding <= kTile - 2
// nonzeros, streams their values / column indices fully coalesced (every lane
// busy, whatever the row lengths), parks the products in LDS and then sums one
// row per lane.  gfx950 only.
#pragma once
#include "common.h"

namespace flow {

// Tiles of the kernels that park ONE product per nonzero in LDS (operator kinds
// 0 and 1, the multigrid level kernels): kPairs index pairs per lane; tiles of
// the kernels that park two (kinds 2 and 4): kPairs2.
#ifndef FLOW_SPMV_PAIRS
#define FLOW_SPMV_PAIRS 2
#endif
constexpr int kPairs = FLOW_SPMV_PAIRS;         // nonzero pairs per lane
constexpr int kTile = 2 * kBlock * kPairs;      // LDS products per workgroup
constexpr int kPairs2 = 2;
constexpr int kTile2 = 2 * kBlock * kPairs2;
static_assert(FLOW_SPMV_ROWS_PER_BLOCK == kBlock, "one lane per row");
static_assert(FLOW_SPMV_NNZ_PER_BLOCK == kTile2 - 2, "tile minus alignment slack");

// The rows [r0, r1) of one workgroup (<= kBlock rows, <= kTile - 2 nonzeros), as
// the lanes hold them between the tile's own loads and a product: load() fetches
// the value pairs and column pairs once, row_sum(x, prod) gathers x, parks the
// products in LDS (prod, kTile doubles) and sums row r0 + lane: gather(), park(),
// a barrier, sum().  One load() may be followed by those steps for several x,
// each with a prod of its own (the block product of eigen_kernels.hip): every
// column then has the bits of a product on its own.
struct StreamTile {
  double2 v[kPairs];
  int2 c[kPairs];
  int a, b;          // the lane's row in prod: [a, b)
  int k0, k1, ka;    // the tile's own nonzeros [k0, k1); ka: k0 aligned down

  template <class Early = NoEarly>
  __device__ __forceinline__ void load(int r0, int r1, const int* __restrict__ rowptr,
                                       const int* __restrict__ cols,
                                       const double* __restrict__ vals,
                                       Early early = Early()) {
    k0 = rowptr[r0];
    k1 = rowptr[r1];
    // 16-byte value loads / 8-byte index loads: every lane owns PAIRS pairs of
    // consecutive nonzeros; the tile base is aligned down to an even index (value
    // planes start 16-B aligned and the host caps a block at kTile-2 nonzeros).
    ka = k0 & ~1;
    const int r = r0 + threadIdx.x;
    early(r, r < r1);
    a = 0;
    b = 0;
    if (r < r1) {
      a = rowptr[r] - ka;
      b = rowptr[r + 1] - ka;
    }
    const double2* __restrict__ v2p = reinterpret_cast<const double2*>(vals + ka);
    const int2* __restrict__ c2p = reinterpret_cast<const int2*>(cols + ka);
    const int npair = (k1 - ka + 1) >> 1;   // a trailing odd element reads one
                                            // entry of the next tile (unused)
#pragma unroll
    for (int j = 0; j < kPairs; ++j) {
      const int p = threadIdx.x + j * kBlock;
      const bool ok = p < npair;
      v[j] = ok ? v2p[p] : make_double2(0.0, 0.0);
      c[j] = ok ? c2p[p] : make_int2(0, 0);
    }
  }

  // x at the lane's nonzeros (x0: the even, x1: the odd entry of each pair)
  struct Gathered {
    double x0[kPairs], x1[kPairs];
  };
  __device__ __forceinline__ Gathered gather(const int* __restrict__ cols,
                                             const double* __restrict__ x) const {
    Gathered g;
    // x is only gathered for the tile's OWN nonzeros [k0, k1): the alignment
    // slack before k0, the odd element behind k1 (a column of another row, or
    // the padding 0 behind the last nonzero) and the idle lanes must not be
    // dereferenced -- x may be a window of a larger vector (row-sharded solves
    // pass x shifted to global row numbering: x[0] is then far outside it)
    // Those entries gather the tile's first column instead (an index select,
    // the loads themselves stay unconditional and all in flight).
    const int lo = k0 - ka, hi = k1 - ka;
    const int safe = cols[k0 < k1 ? k0 : (k0 > 0 ? k0 - 1 : 0)];
    if (k0 < k1) {                       // (block-uniform)
#pragma unroll
      for (int j = 0; j < kPairs; ++j) {   // all gathers in flight before any use
        const int e = 2 * (threadIdx.x + j * kBlock);
        g.x0[j] = x[(e >= lo && e < hi) ? c[j].x : safe];
        g.x1[j] = x[(e + 1 < hi) ? c[j].y : safe];
      }
    } else {
#pragma unroll
      for (int j = 0; j < kPairs; ++j) g.x0[j] = g.x1[j] = 0.0;
    }
    return g;
  }

  // the lane's products into LDS (prod: kTile doubles)
  __device__ __forceinline__ void park(const Gathered& g,
                                       double* __restrict__ prod) const {
    const int npair = (k1 - ka + 1) >> 1;
#pragma unroll
    for (int j = 0; j < kPairs; ++j) {
      const int p = threadIdx.x + j * kBlock;
      if (p < npair) {
        prod[2 * p] = v[j].x * g.x0[j];
        prod[2 * p + 1] = v[j].y * g.x1[j];
      }
    }
  }

  // the lane's row out of the parked products (behind a barrier)
  __device__ __forceinline__ double sum(const double* __restrict__ prod) const {
    double s = 0.0;
    for (int k = a; k < b; ++k) s += prod[k];
    return s;
  }

  __device__ __forceinline__ double row_sum(const int* __restrict__ cols,
                                            const double* __restrict__ x,
                                            double* __restrict__ prod) const {
    const Gathered g = gather(cols, x);
    park(g, prod);
    __syncthreads();
    return sum(prod);
  }
};

// The same tile with a SECOND value plane over the same pattern (the two planes
// of a coupling pair of a mixed operator, mixed_kernels.hip): load() fetches
// the column pairs once and the value pairs of both planes; gather() is the
// tile's own, and plane(p) is the StreamTile of plane p -- its park() and sum()
// are StreamTile's, so each plane has the bits of a product on its own.
struct StreamTilePlanes : StreamTile {
  double2 w[kPairs];   // the second plane's value pairs

  __device__ __forceinline__ void load(int r0, int r1, const int* __restrict__ rowptr,
                                       const int* __restrict__ cols,
                                       const double* __restrict__ vals0,
                                       const double* __restrict__ vals1) {
    StreamTile::load(r0, r1, rowptr, cols, vals0);
    // (the pairs of StreamTile::load: base aligned down, trailing odd element)
    const double2* __restrict__ w2p = reinterpret_cast<const double2*>(vals1 + ka);
    const int npair = (k1 - ka + 1) >> 1;
#pragma unroll
    for (int j = 0; j < kPairs; ++j) {
      const int p = threadIdx.x + j * kBlock;
      w[j] = p < npair ? w2p[p] : make_double2(0.0, 0.0);
    }
  }

  __device__ __forceinline__ StreamTile plane(int p) const {
    StreamTile t = *this;
    if (p) {
#pragma unroll
      for (int j = 0; j < kPairs; ++j) t.v[j] = w[j];
    }
    return t;
  }
};

// The products of the rows [r0, r1) with x go through LDS (prod, kTile doubles),
// then lane i sums row r0 + i.  Returns that row's sum (0 for a lane without a
// row).
template <class Early = NoEarly>
__device__ __forceinline__ double stream_rows_sum(
    int r0, int r1, const int* __restrict__ rowptr, const int* __restrict__ cols,
    const double* __restrict__ vals, const double* __restrict__ x,
    double* __restrict__ prod, Early early = Early()) {
  StreamTile t;
  t.load(r0, r1, rowptr, cols, vals, early);
  return t.row_sum(cols, x, prod);
}

// One tile of the CSR stream -- the rows [r0, r1) of workgroup blockIdx.x (XCD-
// aware tile mapping, common.h).  Returns the lane's row sum; r / r1 tell the
// caller whether the lane has a row.
template <class Early = NoEarly>
__device__ __forceinline__ double stream_tile_row_sum(
    const int* __restrict__ rowptr, const int* __restrict__ cols,
    const double* __restrict__ vals, const int* __restrict__ rowblocks,
    const double* __restrict__ x, double* __restrict__ prod, int& r, int& r1,
    Early early = Early()) {
  const int tile = xcd_tile(blockIdx.x, gridDim.x);
  const int r0 = rowblocks[tile];
  r1 = rowblocks[tile + 1];
  r = r0 + threadIdx.x;
  return stream_rows_sum(r0, r1, rowptr, cols, vals, x, prod, early);
}

// The rows [r0, r1) of one workgroup on the tiles of the kernels that park two
// products per nonzero (<= kTile2 - 2 nonzeros), for a 2x2-block operator (kind
// 2: four value planes over the scalar pattern), as the lanes hold them between
// the tile's own loads and a product with a component-blocked vector (x then y,
// n apart): load() fetches the column pairs and the four planes' value pairs
// once; gather(), park(), a barrier and sum() may then follow for several
// vectors, each with two LDS planes of its own (the block product of
// eigen_kernels.hip).  The per-nonzero expressions, the "own columns only" select
// and the order of the row sums are those of spmv_stream_block2_kernel
// (la_kernels.hip), so every vector has the bits of that kernel's product.
struct StreamTile2 {
  double2 vxx[kPairs2], vxy[kPairs2], vyx[kPairs2], vyy[kPairs2];
  int2 c[kPairs2];   // the columns to gather: the tile's own, else its first
  int a, b;          // the lane's row in the LDS planes: [a, b)
  int npair;         // pairs of the tile

  __device__ __forceinline__ void load(int r0, int r1, const int* __restrict__ rowptr,
                                       const int* __restrict__ cols,
                                       const double* __restrict__ pxx,
                                       const double* __restrict__ pxy,
                                       const double* __restrict__ pyx,
                                       const double* __restrict__ pyy) {
    const int k0 = rowptr[r0];
    const int k1 = rowptr[r1];
    const int ka = k0 & ~1;
    const int r = r0 + threadIdx.x;
    a = 0;
    b = 0;
    if (r < r1) {
      a = rowptr[r] - ka;
      b = rowptr[r + 1] - ka;
    }
    npair = (k1 - ka + 1) >> 1;
    // (only the tile's own columns are dereferenced: StreamTile::gather)
    const int safe = cols[k0 < k1 ? k0 : (k0 > 0 ? k0 - 1 : 0)];
    const int2* __restrict__ c2p = reinterpret_cast<const int2*>(cols + ka);
    const double2* __restrict__ qxx = reinterpret_cast<const double2*>(pxx + ka);
    const double2* __restrict__ qxy = reinterpret_cast<const double2*>(pxy + ka);
    const double2* __restrict__ qyx = reinterpret_cast<const double2*>(pyx + ka);
    const double2* __restrict__ qyy = reinterpret_cast<const double2*>(pyy + ka);
    const double2 zero = make_double2(0.0, 0.0);
#pragma unroll
    for (int j = 0; j < kPairs2; ++j) {
      const int p = threadIdx.x + j * kBlock;
      const bool ok = p < npair;
      const int2 cc = ok ? c2p[p] : make_int2(safe, safe);
      vxx[j] = ok ? qxx[p] : zero;
      vxy[j] = ok ? qxy[p] : zero;
      vyx[j] = ok ? qyx[p] : zero;
      vyy[j] = ok ? qyy[p] : zero;
      c[j].x = 2 * p >= k0 - ka ? cc.x : safe;
      c[j].y = 2 * p + 1 < k1 - ka ? cc.y : safe;
    }
  }

  // both components of x at the lane's nonzeros (u: the even, w: the odd entry
  // of each pair; 0: component x, 1: component y)
  struct Gathered {
    double u0[kPairs2], u1[kPairs2], w0[kPairs2], w1[kPairs2];
  };
  __device__ __forceinline__ Gathered gather(const double* __restrict__ x,
                                             int n) const {
    Gathered g;
#pragma unroll
    for (int j = 0; j < kPairs2; ++j) {   // all gathers in flight before any use
      g.u0[j] = x[c[j].x];
      g.u1[j] = x[n + c[j].x];
      g.w0[j] = x[c[j].y];
      g.w1[j] = x[n + c[j].y];
    }
    return g;
  }

  // the lane's products into LDS (prod0, prod1: kTile2 doubles each)
  __device__ __forceinline__ void park(const Gathered& g, double* __restrict__ prod0,
                                       double* __restrict__ prod1) const {
#pragma unroll
    for (int j = 0; j < kPairs2; ++j) {
      const int p = threadIdx.x + j * kBlock;
      if (p < npair) {
        const double2 axx = vxx[j], axy = vxy[j], ayx = vyx[j], ayy = vyy[j];
        const double u0 = g.u0[j], u1 = g.u1[j];
        const double w0 = g.w0[j], w1 = g.w1[j];
        // a x u + b x v as spmv_stream_block2_kernel is compiled: the second
        // product rounded, the first fused into the sum.  Written out, because
        // the compiler's own contraction of a * u + b * v picks either product
        // depending on the kernel around it (it fused the other one in
        // mixed_kernels.hip), and the bits must not.
        prod0[2 * p] = fma(axx.x, u0, axy.x * u1);
        prod1[2 * p] = fma(ayx.x, u0, ayy.x * u1);
        prod0[2 * p + 1] = fma(axx.y, w0, axy.y * w1);
        prod1[2 * p + 1] = fma(ayx.y, w0, ayy.y * w1);
      }
    }
  }

  // the lane's two row sums out of the parked products (behind a barrier)
  __device__ __forceinline__ double2 sum(const double* __restrict__ prod0,
                                         const double* __restrict__ prod1) const {
    double s0 = 0.0, s1 = 0.0;
    for (int k = a; k < b; ++k) {
      s0 += prod0[k];
      s1 += prod1[k];
    }
    return make_double2(s0, s1);
  }
};

// The same tile with ONE value plane applied to both components of a
// component-blocked vector (component stride xs): the two components' products
// side by side as double2 in LDS (prod: kTile2 double2, 16 KB -- with the
// 1022-nonzero tile that still leaves the 8 workgroups per CU the wave limit
// allows), both row sums out of ONE pass over the segment.  A block of a square
// operator is never empty.  Returns (sum of component 0, sum of component 1).
template <class Early = NoEarly>
__device__ __forceinline__ double2 stream_tile_pair_row_sum(
    const int* __restrict__ rowptr, const int* __restrict__ cols,
    const double* __restrict__ vals, const int* __restrict__ rowblocks,
    const double* __restrict__ x, int xs, double2* __restrict__ prod, int& r,
    int& r1, Early early = Early()) {
  const int tile = xcd_tile(blockIdx.x, gridDim.x);
  const int r0 = rowblocks[tile];
  r1 = rowblocks[tile + 1];
  const int k0 = rowptr[r0];
  const int k1 = rowptr[r1];
  const int ka = k0 & ~1;
  r = r0 + threadIdx.x;
  early(r, r < r1);
  int a = 0, b = 0;
  if (r < r1) {
    a = rowptr[r] - ka;
    b = rowptr[r + 1] - ka;
  }
  const double2* __restrict__ v2p = reinterpret_cast<const double2*>(vals + ka);
  const int2* __restrict__ c2p = reinterpret_cast<const int2*>(cols + ka);
  const int npair = (k1 - ka + 1) >> 1;
  double2 v[kPairs2];
  int2 c[kPairs2];
#pragma unroll
  for (int j = 0; j < kPairs2; ++j) {
    const int p = threadIdx.x + j * kBlock;
    const bool ok = p < npair;
    v[j] = ok ? v2p[p] : make_double2(0.0, 0.0);
    c[j] = ok ? c2p[p] : make_int2(0, 0);
  }
  // (only the tile's own columns are dereferenced: see stream_tile_row_sum)
  const int lo = k0 - ka, hi = k1 - ka;
  const int safe = cols[k0];
  double xa[kPairs2], xb[kPairs2], ua[kPairs2], ub[kPairs2];
#pragma unroll
  for (int j = 0; j < kPairs2; ++j) {   // all gathers in flight before any use
    const int e = 2 * (threadIdx.x + j * kBlock);
    const int cx = (e >= lo && e < hi) ? c[j].x : safe;
    const int cy = (e + 1 < hi) ? c[j].y : safe;
    xa[j] = x[cx];
    xb[j] = x[cy];
    ua[j] = x[xs + cx];
    ub[j] = x[xs + cy];
  }
#pragma unroll
  for (int j = 0; j < kPairs2; ++j) {
    const int p = threadIdx.x + j * kBlock;
    if (p < npair) {
      prod[2 * p] = make_double2(v[j].x * xa[j], v[j].x * ua[j]);
      prod[2 * p + 1] = make_double2(v[j].y * xb[j], v[j].y * ub[j]);
    }
  }
  __syncthreads();
  double s0 = 0.0, s1 = 0.0;
  for (int k = a; k < b; ++k) {
    const double2 q = prod[k];
    s0 += q.x;
    s1 += q.y;
  }
  return make_double2(s0, s1);
}

}  // namespace flow
