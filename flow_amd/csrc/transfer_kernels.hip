// Transfer of discrete fields between spaces and meshes (flow_amd/fem/
// transfer.py): the two kernels behind fem.Transfer.
//
//   flow_nearest_cells   for target nodes that flow_locate_points found in no
//                        cell of the source mesh: the nearest point of the mesh,
//                        which lies on a boundary facet.  One lane per point; a
//                        bucket grid over the boundary facets (layout of
//                        flow_point_grid, built on the host once per mesh) is
//                        searched ring by ring outward from the point's own
//                        bucket until no facet of a farther ring can come
//                        closer than the best one found.  The answer is that of
//                        the search over ALL boundary facets: smallest squared
//                        distance, then lowest facet index.  Contraction stays
//                        off in the distance, so that numpy's evaluation of the
//                        same expressions (tests/transfer_reference.py) gives
//                        the same bits and decides ties alike.
//   flow_transfer_apply  out[a][i] = sum_l phi_l(bary[., i]) u[a][cell_dofs[l][
//                        cell[i]]]: one lane per target node, the P1 / P2 basis
//                        of fem_device.h computed once per node and reused for
//                        all components.  A gather bounded by memory traffic:
//                        cell / bary / out are coalesced streams, the source
//                        reads are scattered (local where the target numbering
//                        is).  No interpreter, no atomics, no LDS: two calls
//                        give the same bits.
#include <cmath>

#include "fem_device.h"

namespace flow {
namespace {

// squared distance of (px, py) to the segment a-b and the parameter t in
// [0, 1] of the foot point a + t (b - a); every operation rounds once
__device__ __forceinline__ double segment_distance2(double ax, double ay, double bx,
                                                    double by, double px, double py,
                                                    double& t) {
#pragma clang fp contract(off)
  const double dx = bx - ax, dy = by - ay;
  const double qx = px - ax, qy = py - ay;
  const double den = dx * dx + dy * dy;
  double s = (qx * dx + qy * dy) / den;
  s = s >= 0.0 ? (s <= 1.0 ? s : 1.0) : 0.0;      // NaN (den == 0): 0, the end a
  const double ex = qx - s * dx, ey = qy - s * dy;
  t = s;
  return ex * ex + ey * ey;
}

// one point per lane; points that have a cell keep it
__global__ __launch_bounds__(kBlock) void nearest_cells_kernel(
    int nc, const double* __restrict__ xy, const flow_point_grid G, int nfacets,
    const int* __restrict__ facet_cell, const int* __restrict__ facet_local, int n,
    const double* __restrict__ pts, int* __restrict__ cell,
    double* __restrict__ bary, double* __restrict__ dist) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (cell[i] != -1) {
    dist[i] = 0.0;
    return;
  }
  const double px = pts[i], py = pts[static_cast<size_t>(n) + i];
  // the point in bucket units; its own bucket clamped as in locate_point (a
  // NaN or a far point never becomes an int out of range)
  const double tx = (px - G.x0) * G.hx_inv, ty = (py - G.y0) * G.hy_inv;
  const double cx = tx >= 0.0 ? (tx <= G.nx - 1.0 ? tx : G.nx - 1.0) : 0.0;
  const double cy = ty >= 0.0 ? (ty <= G.ny - 1.0 ? ty : G.ny - 1.0) : 0.0;
  const int bx = static_cast<int>(floor(cx)), by = static_cast<int>(floor(cy));
  const double wx = 1.0 / G.hx_inv, wy = 1.0 / G.hy_inv;
  // rounding of the bucket arithmetic against the distances: far below a
  // bucket, far above an ulp of the coordinates
  const double slack = 1.0e-9 * (wx + wy);
  double best = INFINITY, best_t = 0.0;
  int best_f = -1;
  const int rings = G.nx > G.ny ? G.nx : G.ny;
  for (int r = 0; r < rings; ++r) {
    const int i0 = bx - r, i1 = bx + r, j0 = by - r, j1 = by + r;
    for (int j = j0 > 0 ? j0 : 0, je = j1 < G.ny - 1 ? j1 : G.ny - 1; j <= je; ++j) {
      const bool row = j == j0 || j == j1;       // a full row of the ring
      const int step = row ? 1 : (i1 - i0 > 0 ? i1 - i0 : 1);
      for (int ii = i0; ii <= i1; ii += step) {
        if (ii < 0 || ii >= G.nx) continue;
        const int b = j * G.nx + ii;
        for (int k = G.start[b], e = G.start[b + 1]; k < e; ++k) {
          const int f = G.cells[k];
          if (f < 0 || f >= nfacets) continue;
          const int c = facet_cell[f], lf = facet_local[f];
          if (c < 0 || c >= nc || lf < 0 || lf > 2) continue;
          const int a = facet_v0(lf), bb = facet_v1(lf);
          double t;
          const double d2 = segment_distance2(
              xy[a * nc + c], xy[(3 + a) * nc + c], xy[bb * nc + c],
              xy[(3 + bb) * nc + c], px, py, t);
          if (d2 < best || (d2 == best && f < best_f)) {
            best = d2;
            best_f = f;
            best_t = t;
          }
        }
      }
    }
    // every facet with a point in the rings searched so far has been seen;
    // the others lie beyond one of the sides of the ring's rectangle that
    // have buckets behind them: nearer than that no point of theirs can be
    double bound = INFINITY;
    if (i0 > 0) bound = fmin(bound, (tx - i0) * wx);
    if (i1 < G.nx - 1) bound = fmin(bound, (i1 + 1 - tx) * wx);
    if (j0 > 0) bound = fmin(bound, (ty - j0) * wy);
    if (j1 < G.ny - 1) bound = fmin(bound, (j1 + 1 - ty) * wy);
    if (bound == INFINITY) break;                // the whole grid is searched
    bound -= slack;
    if (bound > 0.0 && bound * bound > best) break;
  }
  if (best_f < 0) {
    dist[i] = __builtin_nan("");
    return;                                      // no facet: cell stays -1
  }
  const int lf = facet_local[best_f];
  double L[3] = {0.0, 0.0, 0.0};
  L[facet_v0(lf)] = 1.0 - best_t;
  L[facet_v1(lf)] = best_t;
  cell[i] = facet_cell[best_f];
  bary[i] = L[0];
  bary[static_cast<size_t>(n) + i] = L[1];
  bary[2 * static_cast<size_t>(n) + i] = L[2];
  dist[i] = sqrt(best);
}

// one target node per lane, all components.  flow_space does not carry the
// cell count, the stride of cell_dofs: it is vptr[n] / nloc, the length of the
// vector contribution map (a wave-uniform load).
template <int DEG, int NCOMP>
__global__ __launch_bounds__(kBlock) void transfer_apply_kernel(
    const int* __restrict__ cell_dofs, const int* __restrict__ vptr, int n_from,
    int n_to, const int* __restrict__ cell, const double* __restrict__ bary,
    const double* __restrict__ u, double* __restrict__ out) {
  constexpr int NL = Elem<DEG>::NL;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_to) return;
  const int nc = vptr[n_from] / NL;
  const int c = cell[i];
  bool ok = c >= 0 && c < nc;
  int d[NL];
#pragma unroll
  for (int l = 0; l < NL; ++l) {
    d[l] = ok ? cell_dofs[l * nc + c] : 0;
    ok = ok && d[l] >= 0 && d[l] < n_from;
  }
  if (!ok) {
#pragma unroll
    for (int a = 0; a < NCOMP; ++a)
      out[static_cast<size_t>(a) * n_to + i] = __builtin_nan("");
    return;
  }
  const double L[3] = {bary[i], bary[static_cast<size_t>(n_to) + i],
                       bary[2 * static_cast<size_t>(n_to) + i]};
  double phi[NL], dphi[NL][3];
  basis<DEG>(L, phi, dphi);
#pragma unroll
  for (int a = 0; a < NCOMP; ++a) {
    const double* __restrict__ ua = u + static_cast<size_t>(a) * n_from;
    double s = phi[0] * ua[d[0]];
#pragma unroll
    for (int l = 1; l < NL; ++l) s += phi[l] * ua[d[l]];
    out[static_cast<size_t>(a) * n_to + i] = s;
  }
}

int check_mesh(const flow_mesh* mesh) {
  FLOW_REQUIRE(mesh && mesh->nc >= 1 && mesh->xy, "mesh");
  FLOW_REQUIRE(mesh->c1 == 0, "field transfer on strips");
  return FLOW_OK;
}

int check_grid(const flow_point_grid* grid) {
  FLOW_REQUIRE(grid && grid->nx >= 1 && grid->ny >= 1 &&
                   static_cast<long long>(grid->nx) * grid->ny < (1LL << 31) - 1,
               "facet grid size");
  FLOW_REQUIRE(grid->hx_inv > 0.0 && grid->hy_inv > 0.0 && std::isfinite(grid->hx_inv) &&
                   std::isfinite(grid->hy_inv) && std::isfinite(grid->x0) &&
                   std::isfinite(grid->y0),
               "facet grid geometry");
  FLOW_REQUIRE(grid->start && grid->cells, "facet grid arrays");
  return FLOW_OK;
}

}  // namespace
}  // namespace flow

using namespace flow;

extern "C" int flow_nearest_cells(const flow_mesh* mesh, const flow_point_grid* facet_grid,
                                  int nfacets, const int* facet_cell,
                                  const int* facet_local, int n, const double* xy,
                                  int* cell, double* bary, double* dist, void* stream) {
  int rc = check_mesh(mesh);
  if (rc) return rc;
  if ((rc = check_grid(facet_grid))) return rc;
  FLOW_REQUIRE(nfacets >= 1 && facet_cell && facet_local, "boundary facets");
  FLOW_REQUIRE(n >= 0, "point count");
  if (n == 0) return FLOW_OK;
  FLOW_REQUIRE(xy && cell && bary && dist, "pointers");
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(nearest_cells_kernel, dim3((n + kBlock - 1) / kBlock), dim3(kBlock),
                     0, st, mesh->nc, mesh->xy, *facet_grid, nfacets, facet_cell,
                     facet_local, n, xy, cell, bary, dist);
  FLOW_CHECK_LAUNCH();
  return FLOW_OK;
}

extern "C" int flow_transfer_apply(const flow_space* V_from, int ncomp, int n_to,
                                   const int* cell, const double* bary, const double* u,
                                   double* out, void* stream) {
  FLOW_REQUIRE(V_from && (V_from->deg == 1 || V_from->deg == 2) && V_from->n >= 1 &&
                   V_from->cell_dofs && V_from->vptr,
               "source space");
  FLOW_REQUIRE(V_from->r1 == 0, "field transfer on strips");
  FLOW_REQUIRE(ncomp == 1 || ncomp == 2, "components");
  FLOW_REQUIRE(n_to >= 0, "target node count");
  if (n_to == 0) return FLOW_OK;
  FLOW_REQUIRE(cell && bary && u && out, "pointers");
  FLOW_REQUIRE(u != out, "in place");
  hipStream_t st = as_stream(stream);
  const dim3 blocks((n_to + kBlock - 1) / kBlock);
#define FLOW_TRANSFER(DEG, NCOMP)                                                  \
  hipLaunchKernelGGL((transfer_apply_kernel<DEG, NCOMP>), blocks, dim3(kBlock), 0, st, \
                     V_from->cell_dofs, V_from->vptr, V_from->n, n_to, cell, bary, u, out)
  if (V_from->deg == 1) {
    if (ncomp == 1) FLOW_TRANSFER(1, 1);
    else FLOW_TRANSFER(1, 2);
  } else {
    if (ncomp == 1) FLOW_TRANSFER(2, 1);
    else FLOW_TRANSFER(2, 2);
  }
#undef FLOW_TRANSFER
  FLOW_CHECK_LAUNCH();
  return FLOW_OK;
}
