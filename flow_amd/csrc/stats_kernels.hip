// Running time statistics of a field (flow_amd/fem/statistics.py): the two
// streaming kernels behind fem.Statistics.  One sample x (a component-blocked
// dof vector, component a at x + a*n) with weight w taken at time t updates, in
// ONE pass, a store of planes of ld doubles each (ld >= n and even, the store
// 16-byte aligned, so every plane can be read as double2), in this order:
//
//   mean[dim], M2[1 | 3] (covariance), per frequency k: A_k[dim], B_k[dim],
//   min[dim], max[dim], tmin[dim], tmax[dim] (extrema)
//
// Definitions.  Per dof i and component a, with host scalars W' = W + w,
// r = w / W', s = w * W / W':
//
//   delta_a = x_a - mean_a
//   mean_a  = fma(r, delta_a, mean_a)
//   M2_ab   = fma(s * delta_a, delta_b, M2_ab)        (ab = 00; or 00, 01, 11)
//   A_k,a   = fma(w cos phi_k, x_a, A_k,a)
//   B_k,a   = fma(-w sin phi_k, x_a, B_k,a)     phi_k = 2 pi * fmod(f_k * t, 1)
//   if x_a < min_a: min_a = x_a, tmin_a = t      (strict: the first occurrence
//                                                 stays; likewise max)
//
// delta is taken against the mean BEFORE this update.  The first update has
// W = 0, so r = 1 and s = 0: it leaves mean == x bit for bit (x - 0 and
// fma(1, x, 0) are exact; only -0.0 comes out as +0.0) and M2 == 0.0; a
// constant field keeps delta == 0 and with it M2 == 0.0 exactly.  s * delta_a
// and delta_a have the same sign, so a
// diagonal M2 never decreases and never goes below zero.  w cos phi_k and
// -w sin phi_k are formed on the host and arrive by value (flow_stats_freq), as
// do r, s and t: nothing is uploaded.  NaN in x makes the moments NaN; the
// comparisons of the extrema are false for NaN.
//
// flow_stats_merge is Chan's combination of two stores over the same planes,
// with host scalars q = Wb / W, g = Wa * Wb / W, W = Wa + Wb:
//
//   d_a    = mean_b,a - mean_a,a
//   mean_a = fma(q, d_a, mean_a,a)
//   M2_ab  = fma(g * d_a, d_b, M2a_ab + M2b_ab)
//   A, B add;  if min_b < min_a: min_a = min_b, tmin_a = tmin_b  (ties keep a)
//
// Lanes.  One lane per PAIR of dofs (2p, 2p + 1), double2 loads and stores on
// the planes, every component of the pair in registers (delta_0 delta_1 needs
// no second pass); a grid-stride loop over at most kMaxGrid blocks.  The last
// entry of an odd n is handled alone with 8-byte accesses: plane entries at and
// past n (the padding) are never read and never written.  x is read as double2
// where x + a*n is 16-byte aligned and by two 8-byte loads where it is not (the
// second component of a Function with an odd n).  Each lane owns its entries:
// no LDS, no atomics, no reductions -- two identical sequences of calls give
// the same bits.  dim, covariance and extrema are compile-time; the loop over
// the frequencies is wave-uniform.
//
// Bytes moved per update: 8 n dim read (x) plus 16 n * (planes in use) (every
// plane read and written once); planes in use = dim + (covariance ? (dim == 1
// ? 1 : 3) : 0) + 2 dim nfreq + (extrema ? 4 dim : 0).  A merge moves 24 n *
// planes.  Two flops per 16 bytes at best: bound by HBM.
#include <cstdint>

#include "common.h"

#pragma clang fp contract(off)

namespace flow {
namespace {

constexpr int kCov = 1, kExt = 2;       // bits of `flags`

template <bool FULL>
__device__ __forceinline__ double2 load2(const double* p) {
  if (FULL) return *reinterpret_cast<const double2*>(p);
  return make_double2(p[0], 0.0);
}

template <bool FULL>
__device__ __forceinline__ void store2(double* p, double2 v) {
  if (FULL)
    *reinterpret_cast<double2*>(p) = v;
  else
    p[0] = v.x;
}

__device__ __forceinline__ double2 fma2(double a, double2 b, double2 c) {
  return make_double2(fma(a, b.x, c.x), fma(a, b.y, c.y));
}

// number of M2 planes
__host__ __device__ constexpr int cov_planes(int dim, bool cov) {
  return cov ? (dim == 1 ? 1 : 3) : 0;
}

inline int plane_count(int dim, int flags, int nfreq) {
  return dim + cov_planes(dim, flags & kCov) + 2 * dim * nfreq +
         ((flags & kExt) ? 4 * dim : 0);
}

// the entries i (and i + 1 where FULL) of every plane; xal[a]: x + a*n is
// 16-byte aligned (wave-uniform)
template <int DIM, bool COV, bool EXT, bool FULL>
__device__ __forceinline__ void update_entries(size_t i, int n, const bool* xal,
                                               const double* __restrict__ x,
                                               double* __restrict__ P, size_t ld, double r,
                                               double s, double t,
                                               const flow_stats_freq& f) {
  double2 xv[DIM], d[DIM];
#pragma unroll
  for (int a = 0; a < DIM; ++a) {
    const double* xa = x + static_cast<size_t>(a) * n + i;
    if (FULL && xal[a])
      xv[a] = *reinterpret_cast<const double2*>(xa);
    else
      xv[a] = make_double2(xa[0], FULL ? xa[1] : 0.0);
  }
  double* pl = P + i;
#pragma unroll
  for (int a = 0; a < DIM; ++a, pl += ld) {
    double2 m = load2<FULL>(pl);
    d[a] = make_double2(xv[a].x - m.x, xv[a].y - m.y);
    store2<FULL>(pl, fma2(r, d[a], m));
  }
  if (COV) {
#pragma unroll
    for (int a = 0; a < DIM; ++a) {
      const double2 sd = make_double2(s * d[a].x, s * d[a].y);
#pragma unroll
      for (int b = a; b < DIM; ++b, pl += ld) {
        double2 m = load2<FULL>(pl);
        m.x = fma(sd.x, d[b].x, m.x);
        m.y = fma(sd.y, d[b].y, m.y);
        store2<FULL>(pl, m);
      }
    }
  }
  for (int k = 0; k < f.n; ++k) {
    const double c = f.c[k], sn = f.s[k];
#pragma unroll
    for (int a = 0; a < DIM; ++a)
      store2<FULL>(pl + a * ld, fma2(c, xv[a], load2<FULL>(pl + a * ld)));
#pragma unroll
    for (int a = 0; a < DIM; ++a)
      store2<FULL>(pl + (DIM + a) * ld, fma2(sn, xv[a], load2<FULL>(pl + (DIM + a) * ld)));
    pl += 2 * DIM * ld;
  }
  if (EXT) {
#pragma unroll
    for (int a = 0; a < DIM; ++a) {
      double* pmin = pl + a * ld;
      double* ptmin = pl + (2 * DIM + a) * ld;
      double2 v = load2<FULL>(pmin), tv = load2<FULL>(ptmin);
      if (xv[a].x < v.x) { v.x = xv[a].x; tv.x = t; }
      if (xv[a].y < v.y) { v.y = xv[a].y; tv.y = t; }
      store2<FULL>(pmin, v);
      store2<FULL>(ptmin, tv);
      double* pmax = pl + (DIM + a) * ld;
      double* ptmax = pl + (3 * DIM + a) * ld;
      v = load2<FULL>(pmax);
      tv = load2<FULL>(ptmax);
      if (xv[a].x > v.x) { v.x = xv[a].x; tv.x = t; }
      if (xv[a].y > v.y) { v.y = xv[a].y; tv.y = t; }
      store2<FULL>(pmax, v);
      store2<FULL>(ptmax, tv);
    }
  }
}

template <int DIM, bool COV, bool EXT>
__global__ __launch_bounds__(kBlock) void stats_update_kernel(
    int n, const double* __restrict__ x, double* __restrict__ P, size_t ld, double r,
    double s, double t, flow_stats_freq f) {
  bool xal[DIM];
#pragma unroll
  for (int a = 0; a < DIM; ++a)
    xal[a] = (reinterpret_cast<uintptr_t>(x + static_cast<size_t>(a) * n) & 15) == 0;
  const int pairs = n / 2 + (n & 1);
  const int stride = gridDim.x * kBlock;      // <= kMaxGrid * kBlock = 2^19
  for (int p = blockIdx.x * kBlock + threadIdx.x; p < pairs; p += stride) {
    const size_t i = 2 * static_cast<size_t>(p);
    if (i + 1 < static_cast<size_t>(n))
      update_entries<DIM, COV, EXT, true>(i, n, xal, x, P, ld, r, s, t, f);
    else
      update_entries<DIM, COV, EXT, false>(i, n, xal, x, P, ld, r, s, t, f);
  }
}

// A (read and written) and B (read) at the entries i (and i + 1 where FULL)
template <int DIM, bool COV, bool EXT, bool FULL>
__device__ __forceinline__ void merge_entries(size_t i, double* __restrict__ A,
                                              const double* __restrict__ B, size_t ld,
                                              int nfreq, double q, double g) {
  double2 d[DIM];
  double* pa = A + i;
  const double* pb = B + i;
#pragma unroll
  for (int a = 0; a < DIM; ++a, pa += ld, pb += ld) {
    const double2 ma = load2<FULL>(pa), mb = load2<FULL>(pb);
    d[a] = make_double2(mb.x - ma.x, mb.y - ma.y);
    store2<FULL>(pa, fma2(q, d[a], ma));
  }
  if (COV) {
#pragma unroll
    for (int a = 0; a < DIM; ++a) {
      const double2 gd = make_double2(g * d[a].x, g * d[a].y);
#pragma unroll
      for (int b = a; b < DIM; ++b, pa += ld, pb += ld) {
        const double2 va = load2<FULL>(pa), vb = load2<FULL>(pb);
        double2 m = make_double2(va.x + vb.x, va.y + vb.y);
        m.x = fma(gd.x, d[b].x, m.x);
        m.y = fma(gd.y, d[b].y, m.y);
        store2<FULL>(pa, m);
      }
    }
  }
  for (int k = 0; k < 2 * DIM * nfreq; ++k, pa += ld, pb += ld) {
    const double2 va = load2<FULL>(pa), vb = load2<FULL>(pb);
    store2<FULL>(pa, make_double2(va.x + vb.x, va.y + vb.y));
  }
  if (EXT) {
#pragma unroll
    for (int a = 0; a < DIM; ++a) {
      const size_t omin = a * ld, otmin = (2 * DIM + a) * ld;
      double2 v = load2<FULL>(pa + omin), tv = load2<FULL>(pa + otmin);
      double2 w = load2<FULL>(pb + omin), tw = load2<FULL>(pb + otmin);
      if (w.x < v.x) { v.x = w.x; tv.x = tw.x; }
      if (w.y < v.y) { v.y = w.y; tv.y = tw.y; }
      store2<FULL>(pa + omin, v);
      store2<FULL>(pa + otmin, tv);
      const size_t omax = (DIM + a) * ld, otmax = (3 * DIM + a) * ld;
      v = load2<FULL>(pa + omax);
      tv = load2<FULL>(pa + otmax);
      w = load2<FULL>(pb + omax);
      tw = load2<FULL>(pb + otmax);
      if (w.x > v.x) { v.x = w.x; tv.x = tw.x; }
      if (w.y > v.y) { v.y = w.y; tv.y = tw.y; }
      store2<FULL>(pa + omax, v);
      store2<FULL>(pa + otmax, tv);
    }
  }
}

template <int DIM, bool COV, bool EXT>
__global__ __launch_bounds__(kBlock) void stats_merge_kernel(
    int n, double* __restrict__ A, const double* __restrict__ B, size_t ld, int nfreq,
    double q, double g) {
  const int pairs = n / 2 + (n & 1);
  const int stride = gridDim.x * kBlock;
  for (int p = blockIdx.x * kBlock + threadIdx.x; p < pairs; p += stride) {
    const size_t i = 2 * static_cast<size_t>(p);
    if (i + 1 < static_cast<size_t>(n))
      merge_entries<DIM, COV, EXT, true>(i, A, B, ld, nfreq, q, g);
    else
      merge_entries<DIM, COV, EXT, false>(i, A, B, ld, nfreq, q, g);
  }
}

inline bool aligned(const void* p, uintptr_t a) {
  return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0;
}

// do [a, a + na) and [b, b + nb) (in doubles) share an entry?
inline bool overlap(const double* a, size_t na, const double* b, size_t nb) {
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
  return a0 < b0 + 8 * nb && b0 < a0 + 8 * na;
}

inline int pair_grid(int n) { return grid_for(n / 2 + (n & 1), kBlock, kMaxGrid); }

template <int DIM, bool COV, bool EXT>
void launch_update(int n, const double* x, double* P, size_t ld, double r, double s,
                   double t, const flow_stats_freq& f, hipStream_t st) {
  hipLaunchKernelGGL((stats_update_kernel<DIM, COV, EXT>), dim3(pair_grid(n)), dim3(kBlock),
                     0, st, n, x, P, ld, r, s, t, f);
}

template <int DIM, bool COV, bool EXT>
void launch_merge(int n, double* A, const double* B, size_t ld, int nfreq, double q,
                  double g, hipStream_t st) {
  hipLaunchKernelGGL((stats_merge_kernel<DIM, COV, EXT>), dim3(pair_grid(n)), dim3(kBlock),
                     0, st, n, A, B, ld, nfreq, q, g);
}

}  // namespace
}  // namespace flow

using namespace flow;

extern "C" int flow_stats_update(int n, int dim, int flags, const flow_stats_freq* freq,
                                 double r, double s, double t, const double* x,
                                 double* planes, size_t ld, void* stream) {
  FLOW_REQUIRE(n >= 0 && (dim == 1 || dim == 2) && flags >= 0 && flags <= 3,
               "stats update: n >= 0, dim 1 or 2, flags 0..3");
  if (n == 0) return FLOW_OK;
  flow_stats_freq f;
  f.n = 0;
  for (int k = 0; k < FLOW_STATS_MAX_FREQ; ++k) f.c[k] = f.s[k] = 0.0;
  if (freq) {
    FLOW_REQUIRE(freq->n >= 0 && freq->n <= FLOW_STATS_MAX_FREQ,
                 "stats update: at most FLOW_STATS_MAX_FREQ frequencies");
    f = *freq;
  }
  FLOW_REQUIRE(x && planes, "stats update pointers");
  FLOW_REQUIRE(ld >= static_cast<size_t>(n) && ld % 2 == 0, "stats update: ld >= n, even");
  FLOW_REQUIRE(aligned(planes, 16) && aligned(x, 8),
               "stats update: planes 16-byte aligned, x 8-byte aligned");
  const size_t span = static_cast<size_t>(plane_count(dim, flags, f.n) - 1) * ld + n;
  FLOW_REQUIRE(!overlap(planes, span, x, static_cast<size_t>(dim) * n),
               "stats update: x overlaps the planes");
  hipStream_t st = as_stream(stream);
  switch (4 * (dim - 1) + flags) {
    case 0: launch_update<1, false, false>(n, x, planes, ld, r, s, t, f, st); break;
    case 1: launch_update<1, true, false>(n, x, planes, ld, r, s, t, f, st); break;
    case 2: launch_update<1, false, true>(n, x, planes, ld, r, s, t, f, st); break;
    case 3: launch_update<1, true, true>(n, x, planes, ld, r, s, t, f, st); break;
    case 4: launch_update<2, false, false>(n, x, planes, ld, r, s, t, f, st); break;
    case 5: launch_update<2, true, false>(n, x, planes, ld, r, s, t, f, st); break;
    case 6: launch_update<2, false, true>(n, x, planes, ld, r, s, t, f, st); break;
    default: launch_update<2, true, true>(n, x, planes, ld, r, s, t, f, st); break;
  }
  FLOW_CHECK_LAUNCH();
  return FLOW_OK;
}

extern "C" int flow_stats_merge(int n, int dim, int flags, int nfreq, double q, double g,
                                double* planes, const double* other, size_t ld,
                                void* stream) {
  FLOW_REQUIRE(n >= 0 && (dim == 1 || dim == 2) && flags >= 0 && flags <= 3,
               "stats merge: n >= 0, dim 1 or 2, flags 0..3");
  if (n == 0) return FLOW_OK;
  FLOW_REQUIRE(nfreq >= 0 && nfreq <= FLOW_STATS_MAX_FREQ,
               "stats merge: at most FLOW_STATS_MAX_FREQ frequencies");
  FLOW_REQUIRE(planes && other, "stats merge pointers");
  FLOW_REQUIRE(ld >= static_cast<size_t>(n) && ld % 2 == 0, "stats merge: ld >= n, even");
  FLOW_REQUIRE(aligned(planes, 16) && aligned(other, 16),
               "stats merge: both stores 16-byte aligned");
  const size_t span = static_cast<size_t>(plane_count(dim, flags, nfreq) - 1) * ld + n;
  FLOW_REQUIRE(!overlap(planes, span, other, span), "stats merge: the stores overlap");
  hipStream_t st = as_stream(stream);
  switch (4 * (dim - 1) + flags) {
    case 0: launch_merge<1, false, false>(n, planes, other, ld, nfreq, q, g, st); break;
    case 1: launch_merge<1, true, false>(n, planes, other, ld, nfreq, q, g, st); break;
    case 2: launch_merge<1, false, true>(n, planes, other, ld, nfreq, q, g, st); break;
    case 3: launch_merge<1, true, true>(n, planes, other, ld, nfreq, q, g, st); break;
    case 4: launch_merge<2, false, false>(n, planes, other, ld, nfreq, q, g, st); break;
    case 5: launch_merge<2, true, false>(n, planes, other, ld, nfreq, q, g, st); break;
    case 6: launch_merge<2, false, true>(n, planes, other, ld, nfreq, q, g, st); break;
    default: launch_merge<2, true, true>(n, planes, other, ld, nfreq, q, g, st); break;
  }
  FLOW_CHECK_LAUNCH();
  return FLOW_OK;
}
