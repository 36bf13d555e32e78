// Conservative (Galerkin) transfer between meshes (flow_amd/fem/projection.py):
// the right-hand side of the L2 projection of a field of one mesh into a
// space of another, b_(a,i) = int phi_i^to u_a^from dx, over the SUPERMESH --
// the intersections of every target cell with the source cells under it.
//
//   flow_project_load  one TARGET cell per lane.  The lane walks its row of the
//                      pair list (pptr / psrc: the source cells whose padded
//                      bounding box overlaps the target cell's, ascending;
//                      built on the host once) and for every source cell
//                        1. brings both triangles to counter-clockwise (the
//                           vertices 1 and 2 change places FOR THE CLIP only:
//                           the barycentric coordinates below keep the cells'
//                           own vertex order),
//                        2. clips the source triangle against the three edge
//                           half-planes of the target triangle (Sutherland-
//                           Hodgman; the inside test is closed, cross >= 0;
//                           the crossing point is p + t (c - p), t = d0 /
//                           (d0 - d1)): at most 6 vertices,
//                        3. fans the polygon from its first vertex and applies
//                           the 7-point degree-5 rule (kQ7L / kQ7W) on every
//                           sub-triangle: phi_i^to u^from has degree <= 4, so
//                           the rule is exact.  The barycentric coordinates of
//                           the sub-triangle's corners in BOTH cells come from
//                           the cells' affine maps; at a quadrature point they
//                           are the rule's combination of those (affine again),
//                      and adds into be[a][i] and the covered area in that
//                      order: no atomics, two calls give the same bits.  Then
//                      scratch[(a*NL + i)*nc + c] = be[a][i] (times cell area /
//                      covered area where the caller scales), coverage[c] =
//                      covered area / cell area, and the gather over vptr /
//                      vsrc of the target space sums scratch into b.
//
// Coincident edges and shared vertices -- the same mesh, nested meshes, the
// domain boundary -- take no branch of their own: a vertex ON a clip line has
// cross = 0 up to rounding and is inside or just outside; either way the piece
// gained or lost is a sliver of area ~ eps * |cell| and contributes as much.
// Triangles that do not overlap leave fewer than 3 vertices and are skipped.
//
// The polygon is indexed at run time, so it lives in LDS, not in a register
// array (which would go to scratch memory): per lane a buffer A of 6 points and
// a buffer B of 5, [slot][lane] doubles, x and y apart -- 2 * 11 * 256 * 8 =
// 45056 B per block.  The source triangle goes to B, the clips run B -> A
// (<= 4 points) -> B (<= 5) -> A (<= 6).  A lane reads and writes its own
// slots only: no barrier.  Every write checks the buffer's capacity (rounding
// can make the sign pattern of a sliver alternate; exact arithmetic cannot).
//
// Guards: a row that leaves the pair list, a source cell outside [0, nc_from)
// or a dof outside its range gives NaN in that target cell's entries and in
// coverage[c], never a read outside the arrays.
//
//   flow_supermesh_norms  error norms and inner products of two fields on
//                      different meshes (flow_amd/fem/supermesh.py), over the
//                      same pairs with the same clip, fan and rule: one TARGET
//                      cell per lane (mesh_b; the source is mesh_a), at every
//                      quadrature point u and grad u in the source cell, w and
//                      grad w in the target cell, and per component
//                        (u - w)^2 and |grad u - grad w|^2   (product = 0)
//                        u w       and grad u . grad w       (product = 1)
//                      into cell_values[c] and cell_values[nc_b + c].  The
//                      integrands have degree <= 4 on every piece: exact.  The
//                      two planes are summed, on request, as the functionals
//                      are (form_kernels.hip): per-block partials of strided
//                      per-lane sums, at most kRedBlocks of them, then one
//                      finishing block per plane.  NaN in both values of a
//                      target cell under the guards above (its own dofs
//                      included).
#include <climits>
#include <cmath>

#include "fem_device.h"

namespace flow {
namespace {

constexpr int kPolyA = 6;     // points of buffer A (the result of the clip)
constexpr int kPolyB = 5;     // points of buffer B

// one cell's vertices and the affine map to its barycentric coordinates
struct Tri {
  double x[3], y[3];
  double x0, y0, j00, j01, j10, j11, inv, det;
};

__device__ __forceinline__ Tri load_tri(const double* __restrict__ xy, int nc, int c) {
  Tri t;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    t.x[k] = xy[k * nc + c];
    t.y[k] = xy[(3 + k) * nc + c];
  }
  t.x0 = t.x[0];
  t.y0 = t.y[0];
  t.j00 = t.x[1] - t.x[0];
  t.j01 = t.x[2] - t.x[0];
  t.j10 = t.y[1] - t.y[0];
  t.j11 = t.y[2] - t.y[0];
  t.det = t.j00 * t.j11 - t.j01 * t.j10;
  t.inv = 1.0 / t.det;
  if (t.det < 0.0) {          // counter-clockwise for the clip
    const double sx = t.x[1], sy = t.y[1];
    t.x[1] = t.x[2];
    t.y[1] = t.y[2];
    t.x[2] = sx;
    t.y[2] = sy;
  }
  return t;
}

// barycentric coordinates of (px, py) in the cell's own vertex order
__device__ __forceinline__ void bary_of(const Tri& t, double px, double py, double L[3]) {
  const double dx = px - t.x0, dy = py - t.y0;
  L[1] = (t.j11 * dx - t.j01 * dy) * t.inv;
  L[2] = (t.j00 * dy - t.j10 * dx) * t.inv;
  L[0] = 1.0 - L[1] - L[2];
}

// Sutherland-Hodgman against the half-plane to the left of a -> b: n points of
// (ix, iy) -> at most cap points of (ox, oy); [slot * kBlock] of this lane
__device__ __forceinline__ int clip_edge(const double* ix, const double* iy, int n,
                                         double ax, double ay, double bx, double by,
                                         double* ox, double* oy, int cap) {
  if (n < 1) return 0;
  const double ex = bx - ax, ey = by - ay;
  double px = ix[(n - 1) * kBlock], py = iy[(n - 1) * kBlock];
  double dp = ex * (py - ay) - ey * (px - ax);
  int m = 0;
#pragma unroll 1
  for (int k = 0; k < n; ++k) {
    const double cx = ix[k * kBlock], cy = iy[k * kBlock];
    const double dc = ex * (cy - ay) - ey * (cx - ax);
    if ((dp >= 0.0) != (dc >= 0.0) && m < cap) {
      const double t = dp / (dp - dc);
      ox[m * kBlock] = px + t * (cx - px);
      oy[m * kBlock] = py + t * (cy - py);
      ++m;
    }
    if (dc >= 0.0 && m < cap) {
      ox[m * kBlock] = cx;
      oy[m * kBlock] = cy;
      ++m;
    }
    px = cx;
    py = cy;
    dp = dc;
  }
  return m;
}

// the source triangle S clipped to the target triangle T (both counter-
// clockwise): the polygon's vertex count, its points in (ax, ay)
__device__ __forceinline__ int clip_pair(const Tri& T, const Tri& S, double* ax,
                                         double* ay, double* bx, double* by) {
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    bx[k * kBlock] = S.x[k];
    by[k * kBlock] = S.y[k];
  }
  int n = clip_edge(bx, by, 3, T.x[0], T.y[0], T.x[1], T.y[1], ax, ay, kPolyA);
  n = clip_edge(ax, ay, n, T.x[1], T.y[1], T.x[2], T.y[2], bx, by, kPolyB);
  return clip_edge(bx, by, n, T.x[2], T.y[2], T.x[0], T.y[0], ax, ay, kPolyA);
}

// the row of target cell c in the pair list, or an empty one and ok = false
__device__ __forceinline__ void pair_row(const int* __restrict__ pptr, int npairs, int c,
                                         int& p0, int& p1, bool& ok) {
  p0 = pptr[c];
  p1 = pptr[c + 1];
  ok = p0 >= 0 && p0 <= p1 && p1 <= npairs;
  if (!ok) p0 = p1 = 0;
}

#define FLOW_POLY_LDS()                                               \
  __shared__ double poly_x[(kPolyA + kPolyB) * kBlock];               \
  __shared__ double poly_y[(kPolyA + kPolyB) * kBlock];               \
  double* const ax = poly_x + threadIdx.x;                            \
  double* const ay = poly_y + threadIdx.x;                            \
  double* const bx = ax + kPolyA * kBlock;                            \
  double* const by = ay + kPolyA * kBlock

// the geometry alone: coverage[c]
__global__ __launch_bounds__(kBlock) void project_coverage_kernel(
    int nc_from, const double* __restrict__ xy_from, int nc_to,
    const double* __restrict__ xy_to, const int* __restrict__ pptr,
    const int* __restrict__ psrc, int npairs, double* __restrict__ coverage) {
  FLOW_POLY_LDS();
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nc_to) return;
  const Tri T = load_tri(xy_to, nc_to, c);
  int p0, p1;
  bool ok;
  pair_row(pptr, npairs, c, p0, p1, ok);
  double covered = 0.0;
#pragma unroll 1
  for (int t = p0; t < p1; ++t) {
    const int s = psrc[t];
    if (s < 0 || s >= nc_from) {
      ok = false;
      continue;
    }
    const Tri S = load_tri(xy_from, nc_from, s);
    const int n = clip_pair(T, S, ax, ay, bx, by);
    const double x0 = ax[0], y0 = ay[0];
#pragma unroll 1
    for (int k = 1; k + 1 < n; ++k) {
      const double x1 = ax[k * kBlock], y1 = ay[k * kBlock];
      const double x2 = ax[(k + 1) * kBlock], y2 = ay[(k + 1) * kBlock];
      covered += 0.5 * ((x1 - x0) * (y2 - y0) - (x2 - x0) * (y1 - y0));
    }
  }
  coverage[c] = ok ? covered / (0.5 * fabs(T.det)) : __builtin_nan("");
}

template <int DF, int DT, int NCOMP>
__global__ __launch_bounds__(kBlock) void project_load_kernel(
    int nc_from, const double* __restrict__ xy_from, const int* __restrict__ cd_from,
    int n_from, int nc_to, const double* __restrict__ xy_to,
    const int* __restrict__ pptr, const int* __restrict__ psrc, int npairs,
    const double* __restrict__ u, int scale, double* __restrict__ scratch,
    double* __restrict__ coverage) {
  constexpr int NF = Elem<DF>::NL, NT = Elem<DT>::NL;
  FLOW_POLY_LDS();
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nc_to) return;
  const Tri T = load_tri(xy_to, nc_to, c);
  int p0, p1;
  bool ok;
  pair_row(pptr, npairs, c, p0, p1, ok);
  double be[NCOMP][NT];
#pragma unroll
  for (int a = 0; a < NCOMP; ++a)
#pragma unroll
    for (int i = 0; i < NT; ++i) be[a][i] = 0.0;
  double covered = 0.0;
#pragma unroll 1
  for (int t = p0; t < p1; ++t) {
    const int s = psrc[t];
    if (s < 0 || s >= nc_from) {
      ok = false;
      continue;
    }
    const Tri S = load_tri(xy_from, nc_from, s);
    const int n = clip_pair(T, S, ax, ay, bx, by);
    if (n < 3) continue;
    double U[NCOMP][NF];
#pragma unroll
    for (int l = 0; l < NF; ++l) {
      const int dl = cd_from[l * nc_from + s];
      const bool in = dl >= 0 && dl < n_from;
      ok = ok && in;
      const int d = in ? dl : 0;
#pragma unroll
      for (int a = 0; a < NCOMP; ++a) U[a][l] = u[static_cast<size_t>(a) * n_from + d];
    }
    // corner 0 of every sub-triangle of the fan, in both cells
    double Lt[3][3], Ls[3][3];
    const double x0 = ax[0], y0 = ay[0];
    bary_of(T, x0, y0, Lt[0]);
    bary_of(S, x0, y0, Ls[0]);
    double x1 = ax[kBlock], y1 = ay[kBlock];
    bary_of(T, x1, y1, Lt[1]);
    bary_of(S, x1, y1, Ls[1]);
#pragma unroll 1
    for (int k = 2; k < n; ++k) {
      const double x2 = ax[k * kBlock], y2 = ay[k * kBlock];
      bary_of(T, x2, y2, Lt[2]);
      bary_of(S, x2, y2, Ls[2]);
      const double area = 0.5 * ((x1 - x0) * (y2 - y0) - (x2 - x0) * (y1 - y0));
      covered += area;
#pragma unroll
      for (int q = 0; q < 7; ++q) {
        double lt[3], ls[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          lt[j] = kQ7L[q][0] * Lt[0][j] + kQ7L[q][1] * Lt[1][j] + kQ7L[q][2] * Lt[2][j];
          ls[j] = kQ7L[q][0] * Ls[0][j] + kQ7L[q][1] * Ls[1][j] + kQ7L[q][2] * Ls[2][j];
        }
        double phi[NT], dphi[NT][3];
        basis<DT>(lt, phi, dphi);
        const double w = kQ7W[q] * area;
#pragma unroll
        for (int a = 0; a < NCOMP; ++a) {
          const double wu = w * eval_at<DF>(U[a], ls);
#pragma unroll
          for (int i = 0; i < NT; ++i) be[a][i] += wu * phi[i];
        }
      }
      x1 = x2;
      y1 = y2;
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        Lt[1][j] = Lt[2][j];
        Ls[1][j] = Ls[2][j];
      }
    }
  }
  const double cell = 0.5 * fabs(T.det);
  const double nan = __builtin_nan("");
  // scale: the mean over the covered part stands for the rest (covered == 0
  // gives NaN: the caller refuses such cells beforehand)
  const double f = ok ? (scale ? cell / covered : 1.0) : nan;
#pragma unroll
  for (int a = 0; a < NCOMP; ++a)
#pragma unroll
    for (int i = 0; i < NT; ++i)
      scratch[(static_cast<size_t>(a) * NT + i) * nc_to + c] = ok ? be[a][i] * f : nan;
  coverage[c] = ok ? covered / cell : nan;
}

// the physical gradient of sum_j U[j] phi_j at the barycentric point L of the
// cell t (its own vertex order; lambda_0 = 1 - lambda_1 - lambda_2)
template <int DEG>
__device__ __forceinline__ void grad_at(const Tri& t, const double U[Elem<DEG>::NL],
                                        const double L[3], double g[2]) {
  double r[3];
  ref_gradient<DEG>(U, L, r);
  const double a = (r[1] - r[0]) * t.inv, b = (r[2] - r[0]) * t.inv;
  g[0] = a * t.j11 - b * t.j10;
  g[1] = b * t.j00 - a * t.j01;
}

// the nodal values of cell c (NaN-free: a dof outside [0, n) reads dof 0 and
// clears ok)
template <int NL, int NCOMP>
__device__ __forceinline__ void load_cell_values(const int* __restrict__ cd, int nc, int c,
                                                 int n, const double* __restrict__ u,
                                                 double U[NCOMP][NL], bool& ok) {
#pragma unroll
  for (int l = 0; l < NL; ++l) {
    const int dl = cd[l * nc + c];
    const bool in = dl >= 0 && dl < n;
    ok = ok && in;
    const int d = in ? dl : 0;
#pragma unroll
    for (int a = 0; a < NCOMP; ++a) U[a][l] = u[static_cast<size_t>(a) * n + d];
  }
}

// u of (mesh_a, V_a) against w of (mesh_b, V_b) on the cells of mesh_b:
// cell_values[c] the value plane, cell_values[nc_b + c] the gradient plane
template <int DA, int DB, int NCOMP>
__global__ __launch_bounds__(kBlock) void supermesh_norms_kernel(
    int nc_a, const double* __restrict__ xy_a, const int* __restrict__ cd_a, int n_a,
    int nc_b, const double* __restrict__ xy_b, const int* __restrict__ cd_b, int n_b,
    const int* __restrict__ pptr, const int* __restrict__ psrc, int npairs,
    const double* __restrict__ u, const double* __restrict__ w, int product,
    double* __restrict__ cell_values) {
  constexpr int NA = Elem<DA>::NL, NB = Elem<DB>::NL;
  FLOW_POLY_LDS();
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nc_b) return;
  const Tri T = load_tri(xy_b, nc_b, c);
  int p0, p1;
  bool ok;
  pair_row(pptr, npairs, c, p0, p1, ok);
  double W[NCOMP][NB];
  load_cell_values<NB, NCOMP>(cd_b, nc_b, c, n_b, w, W, ok);
  double val = 0.0, grd = 0.0;
#pragma unroll 1
  for (int t = p0; t < p1; ++t) {
    const int s = psrc[t];
    if (s < 0 || s >= nc_a) {
      ok = false;
      continue;
    }
    const Tri S = load_tri(xy_a, nc_a, s);
    const int n = clip_pair(T, S, ax, ay, bx, by);
    if (n < 3) continue;
    double U[NCOMP][NA];
    load_cell_values<NA, NCOMP>(cd_a, nc_a, s, n_a, u, U, ok);
    // corner 0 of every sub-triangle of the fan, in both cells
    double Lt[3][3], Ls[3][3];
    const double x0 = ax[0], y0 = ay[0];
    bary_of(T, x0, y0, Lt[0]);
    bary_of(S, x0, y0, Ls[0]);
    double x1 = ax[kBlock], y1 = ay[kBlock];
    bary_of(T, x1, y1, Lt[1]);
    bary_of(S, x1, y1, Ls[1]);
#pragma unroll 1
    for (int k = 2; k < n; ++k) {
      const double x2 = ax[k * kBlock], y2 = ay[k * kBlock];
      bary_of(T, x2, y2, Lt[2]);
      bary_of(S, x2, y2, Ls[2]);
      const double area = 0.5 * ((x1 - x0) * (y2 - y0) - (x2 - x0) * (y1 - y0));
      // (the points in a loop, not unrolled: nothing here folds to a literal,
      // and unrolled the vector instances take all 256 VGPRs -- one wave per
      // SIMD -- against 221 at most this way)
#pragma unroll 1
      for (int q = 0; q < 7; ++q) {
        double lt[3], ls[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          lt[j] = kQ7L[q][0] * Lt[0][j] + kQ7L[q][1] * Lt[1][j] + kQ7L[q][2] * Lt[2][j];
          ls[j] = kQ7L[q][0] * Ls[0][j] + kQ7L[q][1] * Ls[1][j] + kQ7L[q][2] * Ls[2][j];
        }
        const double wq = kQ7W[q] * area;
#pragma unroll
        for (int a = 0; a < NCOMP; ++a) {
          const double uv = eval_at<DA>(U[a], ls), wv = eval_at<DB>(W[a], lt);
          double gu[2], gw[2];
          grad_at<DA>(S, U[a], ls, gu);
          grad_at<DB>(T, W[a], lt, gw);
          if (product) {
            val += wq * (uv * wv);
            grd += wq * (gu[0] * gw[0] + gu[1] * gw[1]);
          } else {
            const double d = uv - wv, d0 = gu[0] - gw[0], d1 = gu[1] - gw[1];
            val += wq * (d * d);
            grd += wq * (d0 * d0 + d1 * d1);
          }
        }
      }
      x1 = x2;
      y1 = y2;
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        Lt[1][j] = Lt[2][j];
        Ls[1][j] = Ls[2][j];
      }
    }
  }
  const double nan = __builtin_nan("");
  cell_values[c] = ok ? val : nan;
  cell_values[static_cast<size_t>(nc_b) + c] = ok ? grd : nan;
}

// fixed-order sums of the planes blockIdx.y of `in` (n entries each): block
// (x, y) leaves the sum of its lanes' strided sums in out[y * out_stride + x].
// Stage 1 over the cells, stage 2 (one block per plane, FINISH) over stage 1's
// partials
template <bool FINISH>
__global__ __launch_bounds__(kBlock) void supermesh_sum_kernel(
    int n, const double* __restrict__ in, size_t in_stride, double* __restrict__ out,
    int out_stride) {
  const double* __restrict__ p = in + blockIdx.y * in_stride;
  double s = 0.0;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    s += FINISH ? load_scalar(p + i) : p[i];
  s = block_sum_once(s);
  if (threadIdx.x == 0) {
    if (FINISH) store_scalar(out + blockIdx.y * out_stride + blockIdx.x, s);
    else out[blockIdx.y * out_stride + blockIdx.x] = s;
  }
}

int check_side(const flow_mesh* mesh, const flow_space* V, const char* what) {
  FLOW_REQUIRE(mesh && mesh->nc >= 1 && mesh->nc <= INT_MAX / 6 && mesh->xy, what);
  FLOW_REQUIRE(mesh->c1 == 0, "field projection on strips");
  if (V) {
    FLOW_REQUIRE((V->deg == 1 || V->deg == 2) && V->n >= 1 && V->cell_dofs, what);
    FLOW_REQUIRE(V->r1 == 0, "field projection on strips");
  }
  return FLOW_OK;
}

}  // namespace
}  // namespace flow

using namespace flow;

extern "C" int flow_project_load(const flow_mesh* mesh_from, const flow_space* V_from,
                                 const flow_mesh* mesh_to, const flow_space* V_to,
                                 int ncomp, const int* pptr, const int* psrc, int npairs,
                                 const double* u, int scale, double* scratch,
                                 double* coverage, double* b, void* stream) {
  int rc = check_side(mesh_from, u ? V_from : nullptr, "source mesh / space");
  if (rc) return rc;
  if ((rc = check_side(mesh_to, u ? V_to : nullptr, "target mesh / space"))) return rc;
  FLOW_REQUIRE(npairs >= 0 && pptr && (psrc || npairs == 0), "pair list");
  FLOW_REQUIRE(coverage, "coverage");
  hipStream_t st = as_stream(stream);
  const int nc = mesh_to->nc;
  const dim3 blocks((nc + kBlock - 1) / kBlock);
  if (!u) {
    // the geometry alone
    hipLaunchKernelGGL(project_coverage_kernel, blocks, dim3(kBlock), 0, st, mesh_from->nc,
                       mesh_from->xy, nc, mesh_to->xy, pptr, psrc, npairs, coverage);
    FLOW_CHECK_LAUNCH();
    return FLOW_OK;
  }
  FLOW_REQUIRE(V_from && V_to, "spaces");
  FLOW_REQUIRE(V_to->vptr && V_to->vsrc, "vector contribution map of the target space");
  FLOW_REQUIRE(ncomp == 1 || ncomp == 2, "components");
  FLOW_REQUIRE(scale == 0 || scale == 1, "scale");
  FLOW_REQUIRE(scratch && b, "pointers");
  FLOW_REQUIRE(u != b && u != scratch && u != coverage && b != scratch && b != coverage &&
                   scratch != coverage,
               "operands that are the same buffer");
#define FLOW_PROJECT(DF, DT, NCOMP)                                                     \
  hipLaunchKernelGGL((project_load_kernel<DF, DT, NCOMP>), blocks, dim3(kBlock), 0, st, \
                     mesh_from->nc, mesh_from->xy, V_from->cell_dofs, V_from->n, nc,    \
                     mesh_to->xy, pptr, psrc, npairs, u, scale, scratch, coverage)
  const int key = (V_from->deg - 1) * 4 + (V_to->deg - 1) * 2 + (ncomp - 1);
  switch (key) {
    case 0: FLOW_PROJECT(1, 1, 1); break;
    case 1: FLOW_PROJECT(1, 1, 2); break;
    case 2: FLOW_PROJECT(1, 2, 1); break;
    case 3: FLOW_PROJECT(1, 2, 2); break;
    case 4: FLOW_PROJECT(2, 1, 1); break;
    case 5: FLOW_PROJECT(2, 1, 2); break;
    case 6: FLOW_PROJECT(2, 2, 1); break;
    default: FLOW_PROJECT(2, 2, 2); break;
  }
#undef FLOW_PROJECT
  FLOW_CHECK_LAUNCH();
  const int nl = V_to->deg == 1 ? 3 : 6;
  return gather(V_to->n, ncomp, V_to->vptr, V_to->vsrc, scratch,
                static_cast<size_t>(nl) * nc, b, st);
}

extern "C" int flow_supermesh_norms(const flow_mesh* mesh_a, const flow_space* V_a,
                                    const flow_mesh* mesh_b, const flow_space* V_b,
                                    int ncomp, const int* pptr, const int* psrc,
                                    int npairs, const double* u, const double* w,
                                    int product, double* cell_values, double* work,
                                    double* totals_host, void* stream) {
  FLOW_REQUIRE(V_a && V_b, "spaces");
  int rc = check_side(mesh_a, V_a, "source mesh / space");
  if (rc) return rc;
  if ((rc = check_side(mesh_b, V_b, "target mesh / space"))) return rc;
  FLOW_REQUIRE(npairs >= 0 && pptr && (psrc || npairs == 0), "pair list");
  FLOW_REQUIRE(ncomp == 1 || ncomp == 2, "components");
  FLOW_REQUIRE(product == 0 || product == 1, "product");
  FLOW_REQUIRE(u && w && cell_values, "pointers");
  FLOW_REQUIRE(work || !totals_host, "totals without a work buffer");
  // (u and w are only read: the same field twice is allowed)
  FLOW_REQUIRE(u != cell_values && w != cell_values && u != work && w != work &&
                   cell_values != work,
               "operands that are the same buffer");
  static_assert(3 * kRedBlocks + 2 <= FLOW_REDUCE_WORK, "work size");
  hipStream_t st = as_stream(stream);
  const int nc = mesh_b->nc;
  const dim3 blocks((nc + kBlock - 1) / kBlock);
#define FLOW_SUPERMESH(DA, DB, NCOMP)                                                      \
  hipLaunchKernelGGL((supermesh_norms_kernel<DA, DB, NCOMP>), blocks, dim3(kBlock), 0, st, \
                     mesh_a->nc, mesh_a->xy, V_a->cell_dofs, V_a->n, nc, mesh_b->xy,       \
                     V_b->cell_dofs, V_b->n, pptr, psrc, npairs, u, w, product,            \
                     cell_values)
  const int key = (V_a->deg - 1) * 4 + (V_b->deg - 1) * 2 + (ncomp - 1);
  switch (key) {
    case 0: FLOW_SUPERMESH(1, 1, 1); break;
    case 1: FLOW_SUPERMESH(1, 1, 2); break;
    case 2: FLOW_SUPERMESH(1, 2, 1); break;
    case 3: FLOW_SUPERMESH(1, 2, 2); break;
    case 4: FLOW_SUPERMESH(2, 1, 1); break;
    case 5: FLOW_SUPERMESH(2, 1, 2); break;
    case 6: FLOW_SUPERMESH(2, 2, 1); break;
    default: FLOW_SUPERMESH(2, 2, 2); break;
  }
#undef FLOW_SUPERMESH
  FLOW_CHECK_LAUNCH();
  if (!totals_host) return FLOW_OK;
  // [0, nparts) and [kRedBlocks, + nparts): the partials of the two planes;
  // the two totals behind them
  const int nparts = grid_for(nc, kBlock, kRedBlocks);
  double* totals = work + 3 * kRedBlocks;
  hipLaunchKernelGGL(supermesh_sum_kernel<false>, dim3(nparts, 2), dim3(kBlock), 0, st, nc,
                     cell_values, static_cast<size_t>(nc), work, kRedBlocks);
  FLOW_CHECK_LAUNCH();
  hipLaunchKernelGGL(supermesh_sum_kernel<true>, dim3(1, 2), dim3(kBlock), 0, st, nparts,
                     work, static_cast<size_t>(kRedBlocks), totals, 1);
  FLOW_CHECK_LAUNCH();
  return flow_read_doubles(totals, 2, totals_host, stream);
}
