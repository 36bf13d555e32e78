// Wall distance by a monotone Eikonal solver on the mesh (flow_amd/fem/
// distance.py): the kernel behind fem.Distance.
//
//   flow_distance_sweeps   nsweeps Jacobi sweeps of
//                            new[i] = min(old[i], min over the triangles at i of
//                                         the Hopf-Lax update of i from them)
//                          between two buffers, on the P1 triangulation of the
//                          dofs (subtri.h).  One lane per dof; a gather: the
//                          lane walks its row of the vector contribution map
//                          (for_each_sub_triangle_at), takes the positions of
//                          each triangle's nodes from the cell's three vertex
//                          coordinates, reads the two other values from `old`
//                          and takes the minimum.
//                          No atomics, no LDS, no private memory (local indices
//                          are turned into values by selects); min is exact and
//                          commutes, so the result does not depend on the order
//                          of the row and two calls give the same bits.
//                          Coalesced: vptr, old[i], new[i]; streamed per lane:
//                          its row of vsrc; scattered (local where the numbering
//                          follows the mesh): the patch cells' coordinates, dof
//                          indices and values.
//
// The update of C from the triangle (C, A, B) with values T_A, T_B (Bornemann
// and Rasch): the minimum over the edge A-B of T(x) + |C - x|, T linear on the
// edge -- the two end points, and the interior stationary point where there is
// one.  An infinite input is skipped, so no inf - inf is formed.  Contraction
// is off: tests/distance_reference.py writes the same expression tree in numpy.
#include "subtri.h"

namespace flow {
namespace {

// min over x on the edge A-B of T(x) + |C - x|; +inf when both inputs are
__device__ __forceinline__ double hopf_lax(double cx, double cy, double ax, double ay,
                                           double bx, double by, double ta, double tb) {
#pragma clang fp contract(off)
  const double inf = __builtin_inf();
  const double ex = ax - bx, ey = ay - by;
  const double px = cx - bx, py = cy - by;
  const double qx = cx - ax, qy = cy - ay;
  const bool fa = ta < inf, fb = tb < inf;
  double best = inf;
  if (fa) {
    const double c = ta + sqrt(qx * qx + qy * qy);
    best = c < best ? c : best;
  }
  if (fb) {
    const double c = tb + sqrt(px * px + py * py);
    best = c < best ? c : best;
  }
  if (fa && fb) {
    const double ee = ex * ex + ey * ey;
    const double le = sqrt(ee);
    const double d = ta - tb;
    if (fabs(d) < le) {
      const double s = (ex * px + ey * py) / ee;
      const double h = fabs(ex * py - ey * px) / le;
      const double t = h * d / sqrt(ee - d * d);
      const double lam = s - t / le;
      // (a NaN or an infinity from ee - d*d <= 0 in rounding fails the test)
      if (lam >= 0.0 && lam <= 1.0) {
        const double c = tb + lam * d + sqrt(t * t + h * h);
        best = c < best ? c : best;
      }
    }
  }
  return best;
}

// one lane per dof
template <int DEG>
__global__ __launch_bounds__(kBlock) void distance_sweep_kernel(
    int nc, const double* __restrict__ xy, const int* __restrict__ cell_dofs, int n,
    const int* __restrict__ vptr, const int* __restrict__ vsrc,
    const double* __restrict__ old, double* __restrict__ out, int* __restrict__ flag) {
  const int node = blockIdx.x * blockDim.x + threadIdx.x;
  if (node >= n) return;
  const double mine = old[node];
  double best = mine;
  bool ok = true;
  for_each_sub_triangle_at<DEG>(
      node, nc, n, cell_dofs, vptr, vsrc, ok,
      [&](int i, int c, int la, int lb, int da, int db, bool in) {
        const double x0 = xy[0 * nc + c], x1 = xy[1 * nc + c], x2 = xy[2 * nc + c];
        const double y0 = xy[3 * nc + c], y1 = xy[4 * nc + c], y2 = xy[5 * nc + c];
        const double ta = old[in ? da : 0], tb = old[in ? db : 0];
        const double cand = hopf_lax(
            node_coord(i, x0, x1, x2), node_coord(i, y0, y1, y2),
            node_coord(la, x0, x1, x2), node_coord(la, y0, y1, y2),
            node_coord(lb, x0, x1, x2), node_coord(lb, y0, y1, y2), ta, tb);
        best = cand < best ? cand : best;
      });
  out[node] = ok ? best : __builtin_nan("");
  // every lane that lowered its value stores the same 1: a plain vector store
  if (flag != nullptr && ok && best < mine) *flag = 1;
}

}  // namespace
}  // namespace flow

using namespace flow;

extern "C" int flow_distance_sweeps(const flow_mesh* mesh, const flow_space* V,
                                    int nsweeps, double* buf_a, double* buf_b,
                                    int* flag, void* stream) {
  const int rc = check_p12_mesh_space(mesh, V, "wall distance on strips", true);
  if (rc) return rc;
  hipStream_t st = as_stream(stream);
  const dim3 blocks((V->n + kBlock - 1) / kBlock);
  return jacobi_sweeps(V, nsweeps, buf_a, buf_b, flag,
                       [&](const double* src, double* dst, int* f) {
                         FLOW_LAUNCH_BY_DEGREE(V->deg, distance_sweep_kernel, blocks, st,
                                               mesh->nc, mesh->xy, V->cell_dofs, V->n,
                                               V->vptr, V->vsrc, src, dst, f);
                       });
}
