// The fp16 CSR-stream tile: ONE routine (fp16_tile_row_sum) for the four stream
// formats of the mass solver (mass_kernels.hip) and of the p-multigrid levels
// (pmg_kernels.hip), and what the two share around it -- the tile shape, the
// Chebyshev recurrence, the lowest column of a tile.  gfx950 only.
#pragma once
#include "common.h"

#include <hip/hip_fp16.h>

namespace flow {

constexpr int kQuads16 = 2;                      // quads of nonzeros per lane
constexpr int kTile16 = kBlock * 4 * kQuads16;   // LDS products per workgroup
static_assert(FLOW_PMG_NNZ_PER_BLOCK == kTile16 - 4,
              "tile minus alignment slack (base aligned down to a multiple of 4)");

// fp32 vectors: one float per dof (scalar systems) or the two components
// interleaved (float2: one 8-byte gather per nonzero serves both); a weight is
// one number for both components or one per component
__device__ __forceinline__ float vscale(float w, float g) { return w * g; }
__device__ __forceinline__ float2 vscale(float w, float2 g) {
  return make_float2(w * g.x, w * g.y);
}
__device__ __forceinline__ float2 vscale(float2 w, float2 g) {
  return make_float2(w.x * g.x, w.y * g.y);
}
__device__ __forceinline__ void vadd(float& s, float p) { s += p; }
__device__ __forceinline__ void vadd(float2& s, float2 p) {
  s.x += p.x;
  s.y += p.y;
}
__device__ __forceinline__ void vzero(float& s) { s = 0.f; }
__device__ __forceinline__ void vzero(float2& s) { s = make_float2(0.f, 0.f); }

// ---------------------------------------------------------------------------
// Stream formats.  A format holds the stream's pointers and says how a lane
// loads quad p of the tile whose aligned base is nonzero ka (load; a quad that
// is not loaded holds columns 0), and how nonzero j of a loaded quad yields its
// column (col) and its weight (weight: float, or float2 = one weight per
// component).  base(tile) is the tile's lowest column where the columns are
// 16-bit offsets from it (cbase[tile], read only then; handed to load and col),
// first_col(k0, base) the column of the tile's first nonzero.  All value /
// column arrays are 16-byte aligned and readable three entries past the last
// nonzero.
// ---------------------------------------------------------------------------
template <class H>
struct Vals4 {              // the values of four nonzeros: 8 B (half), 16 B (half2)
  H v[4];
};
static_assert(sizeof(Vals4<__half>) == 8 && sizeof(Vals4<__half2>) == 16,
              "packed quad");
// half(x) of an fp64 value in ONE rounding to nearest even (the setup kernels:
// the scaled entries v * (1 / d)).  Written through float -- half(float(x)) --
// the value would be rounded twice, one fp16 ulp off wherever x lies within
// half a float ulp of a tie of the fp16 grid (2^-13 of all entries), unless the
// compiler folds the two conversions into this one: it does on gfx950, so this
// is what the streams have always held (tests/test_fp16_streams_gpu.py compares
// them bit for bit).
__device__ __forceinline__ __half half_rn(double x) {
  return __half(static_cast<_Float16>(x));
}
__device__ __forceinline__ float widen(__half h) { return __half2float(h); }
__device__ __forceinline__ float2 widen(__half2 h) { return __half22float2(h); }
template <class T4>
__device__ __forceinline__ auto at4(const T4& q, int j) {
  return j == 0 ? q.x : j == 1 ? q.y : j == 2 ? q.z : q.w;
}

// H values + int32 columns: H = __half, ONE plane (6 B per nonzero: the mass
// solver's plain stream), or __half2, a plane per component (8 B: the pmg
// levels whose tiles' columns span 65536 or more)
template <class H>
struct Cols32Stream {
  const H* vals;
  const int* cols;
  struct Quad {
    Vals4<H> v;
    int4 c = {0, 0, 0, 0};
  };
  __device__ __forceinline__ int base(int) const { return 0; }
  __device__ __forceinline__ int first_col(int k0, int) const { return cols[k0]; }
  __device__ __forceinline__ Quad load(int ka, int p, int) const {
    return {reinterpret_cast<const Vals4<H>*>(vals + ka)[p],
            reinterpret_cast<const int4*>(cols + ka)[p]};
  }
  static __device__ __forceinline__ int col(const Quad& w, int j, int) {
    return at4(w.c, j);
  }
  static __device__ __forceinline__ auto weight(const Quad& w, int j) {
    return widen(w.v.v[j]);
  }
};

// half2 values + 16-bit column offsets from the tile's lowest column (cols16 /
// cbase of flow_pmg_level: 6 B per nonzero instead of 8).  The offsets become
// columns as they are loaded: cbase[tile] is then wanted with the tile's first
// loads, not behind the quads.
struct Cols16Stream {
  const __half2* vals;
  const unsigned short* cols16;
  const int* cbase;
  struct Quad {
    Vals4<__half2> v;
    int4 c = {0, 0, 0, 0};
  };
  __device__ __forceinline__ int base(int tile) const { return cbase[tile]; }
  __device__ __forceinline__ int first_col(int k0, int base) const {
    return base + cols16[k0];
  }
  __device__ __forceinline__ Quad load(int ka, int p, int base) const {
    const ushort4 u = reinterpret_cast<const ushort4*>(cols16 + ka)[p];
    return {reinterpret_cast<const Vals4<__half2>*>(vals + ka)[p],
            make_int4(base + u.x, base + u.y, base + u.z, base + u.w)};
  }
  static __device__ __forceinline__ int col(const Quad& w, int j, int) {
    return at4(w.c, j);
  }
  static __device__ __forceinline__ float2 weight(const Quad& w, int j) {
    return widen(w.v.v[j]);
  }
};

// The PACKED stream: one 32-bit word per nonzero -- the fp16 value in the low
// half, the column as a 16-bit offset from cbase[tile] in the high half -- so a
// quad of nonzeros is ONE 16-byte load (4 B per nonzero, half the stream-load
// instructions).  Possible whenever a tile's columns span < 65536 (any banded
// numbering; the host checks and falls back to a plain stream otherwise).
struct PackedStream {
  const unsigned* packed;
  const int* cbase;
  struct Quad {
    uint4 w = {0u, 0u, 0u, 0u};
  };
  __device__ __forceinline__ int base(int tile) const { return cbase[tile]; }
  __device__ __forceinline__ int first_col(int k0, int base) const {
    return base + static_cast<int>(packed[k0] >> 16);
  }
  __device__ __forceinline__ Quad load(int ka, int p, int) const {
    return {reinterpret_cast<const uint4*>(packed + ka)[p]};
  }
  static __device__ __forceinline__ int col(const Quad& w, int j, int base) {
    return base + static_cast<int>(at4(w.w, j) >> 16);
  }
  static __device__ __forceinline__ float weight(const Quad& w, int j) {
    return widen(__ushort_as_half(
        static_cast<unsigned short>(at4(w.w, j) & 0xffffu)));
  }
};

// One tile of an fp16 stream -- rows [r0, r1) of workgroup blockIdx.x (at most
// kBlock rows, kTile16 - 4 nonzeros): every lane loads kQuads16 quads of
// nonzeros from a base aligned down to a multiple of four nonzeros, the
// products weight * g[column] go through LDS (prod: kTile16 entries), lane i
// sums row r0 + i in the order of its nonzeros and returns the sum (r, r1: the
// lane's row and the end of the tile; r >= r1: no row).
//
// Latency.  These kernels are bound by the chain of dependent loads of a tile
// (row blocks -> row pointers -> quads -> gathers; a workgroup lives ~6 us, a
// link of the chain is ~1 us of it), not by bytes: all quads, and all gathers
// behind them, are in flight before the first use, and a tile carries as many
// nonzeros as the LDS products of a workgroup allow (16 KB of float2: still
// eight workgroups per CU).  early(row, has_row) is called as soon as the lane
// knows its row: the caller issues its epilogue's loads there, so that they
// travel with the tile's own loads instead of adding one more link behind the
// row sum.  (NoEarly: common.h)
//
// Window safety.  g may be a window of a vector addressed by global row (the
// strip-sharded solvers, like stream_tile_row_sum of csr_stream.h): it is only
// dereferenced at the columns of the tile's OWN nonzeros [k0, k1).  The
// alignment slack in front of k0, what a quad holds behind k1 and the lanes
// that loaded nothing gather the column of the tile's first nonzero (`safe`)
// instead; an empty tile gathers nothing.  tests/access_model.py
// (quad_tile_accesses) restates exactly this rule.
template <class Fmt, class V, class Early = NoEarly>
__device__ __forceinline__ V fp16_tile_row_sum(
    const int* __restrict__ rowptr, const Fmt fmt,
    const int* __restrict__ rowblocks, const V* __restrict__ g,
    V* __restrict__ prod, int& r, int& r1, Early early = Early()) {
  const int tile = xcd_tile(blockIdx.x, gridDim.x);
  const int r0 = rowblocks[tile];
  r1 = rowblocks[tile + 1];
  const int base = fmt.base(tile);
  const int k0 = rowptr[r0];
  const int k1 = rowptr[r1];
  const int ka = k0 & ~3;
  r = r0 + threadIdx.x;
  early(r, r < r1);
  int a = 0, b = 0;
  if (r < r1) {
    a = rowptr[r] - ka;
    b = rowptr[r + 1] - ka;
  }
  const int lo = k0 - ka, hi = k1 - ka;          // hi <= kTile16 - 1
  typename Fmt::Quad w[kQuads16];
#pragma unroll
  for (int q = 0; q < kQuads16; ++q) {
    const int p = threadIdx.x + q * kBlock;
    if (4 * p < hi) w[q] = fmt.load(ka, p, base);
  }
  if (k0 < k1) {                                   // (block-uniform)
    const int safe = fmt.first_col(k0, base);
    V gg[kQuads16][4];
#pragma unroll
    for (int q = 0; q < kQuads16; ++q) {           // all gathers in flight
      const int e0 = 4 * (threadIdx.x + q * kBlock);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int e = e0 + j;
        gg[q][j] = g[(e >= lo && e < hi) ? Fmt::col(w[q], j, base) : safe];
      }
    }
#pragma unroll
    for (int q = 0; q < kQuads16; ++q) {
      const int e0 = 4 * (threadIdx.x + q * kBlock);
      if (e0 < hi) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          prod[e0 + j] = vscale(Fmt::weight(w[q], j), gg[q][j]);
      }
    }
  }
  __syncthreads();
  V s;
  vzero(s);
  for (int k = a; k < b; ++k) vadd(s, prod[k]);
  return s;
}

// The lowest column of the tile with the nonzeros [k0, k1), on every lane of
// the workgroup: block minimum of cols[k0 .. k1), 0 for an empty tile (setup of
// the 16-bit column offsets: cbase[tile])
__device__ __forceinline__ int tile_lowest_col(const int* __restrict__ cols,
                                               int k0, int k1) {
  __shared__ int wmin[kBlock / 64];
  int m = 0x7fffffff;
  for (int k = k0 + threadIdx.x; k < k1; k += kBlock) m = min(m, cols[k]);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = min(m, __shfl_down(m, off, 64));
  if ((threadIdx.x & 63) == 0) wmin[threadIdx.x >> 6] = m;
  __syncthreads();
  int base = wmin[0];
#pragma unroll
  for (int w = 1; w < kBlock / 64; ++w) base = min(base, wmin[w]);
  return k0 < k1 ? base : 0;
}

// The Chebyshev recurrence on the interval [lo, hi] (host side): d_0 = first()
// * rho_0, then d' = c1 d + c2 rho' with the coefficients of next()
struct Cheb {
  double theta, delta, sigma, rho;
  Cheb(double lo, double hi)
      : theta(0.5 * (hi + lo)), delta(0.5 * (hi - lo)), sigma(theta / delta),
        rho(1.0 / sigma) {}
  float first() const { return static_cast<float>(1.0 / theta); }
  void next(float* c1, float* c2) {
    const double rn = 1.0 / (2.0 * sigma - rho);
    *c1 = static_cast<float>(rn * rho);
    *c2 = static_cast<float>(2.0 * rn / delta);
    rho = rn;
  }
};

}  // namespace flow
