// Wall distance by a monotone Eikonal solver on the mesh (flow_amd/fem/
// distance.py): the kernel behind fem.Distance.
//
//   flow_distance_sweeps   nsweeps Jacobi sweeps of
//                            new[i] = min(old[i], min over the triangles at i of
//                                         the Hopf-Lax update of i from them)
//                          between two buffers.  The graph is the P1
//                          triangulation of the dofs: for P1 the cells, for P2
//                          every cell cut into its three corner triangles
//                          (v_i, e_(i+2), e_(i+1)) and the middle one (e_0, e_1,
//                          e_2), local dofs [v0 v1 v2 e0 e1 e2] with e_i opposite
//                          v_i as in fem_device.h.  One lane per dof; a gather:
//                          the lane walks its row of the vector contribution map
//                          (vptr / vsrc, entry l*nc + c: local node l of cell c),
//                          builds the one triangle (P1, a P2 vertex) or the three
//                          triangles (a P2 edge dof) of that cell that hold the
//                          node -- node positions from the cell's three vertex
//                          coordinates, mid points of the straight edges -- reads
//                          the two other values from `old` and takes the minimum.
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
#include <climits>
#include <cmath>

#include "fem_device.h"

namespace flow {
namespace {

// coordinate of local node m (0-2: the vertices, 3-5: the mid points of the
// edges opposite them) from the three vertex coordinates; selects only
__device__ __forceinline__ double node_coord(int m, double v0, double v1, double v2) {
#pragma clang fp contract(off)
  const double vert = m == 0 ? v0 : (m == 1 ? v1 : v2);
  const double mid = m == 3 ? 0.5 * (v1 + v2) : (m == 4 ? 0.5 * (v0 + v2) : 0.5 * (v0 + v1));
  return m < 3 ? vert : mid;
}

// the k-th triangle of the cell's sub-triangulation that holds local node i:
// its two other local nodes (la, lb), in the triangle's cyclic order behind the
// node (tests/distance_reference.py lists the same triples).  P1 and P2
// vertices have one (k = 0), P2 edge dofs three: the corner triangles at the
// edge's two ends, then the middle.
template <int DEG>
__device__ __forceinline__ void sub_triangle(int i, int k, int& la, int& lb) {
  if constexpr (DEG == 1) {
    la = i == 2 ? 0 : i + 1;
    lb = i == 0 ? 2 : i - 1;
  } else {
    const int e = i < 3 ? i : i - 3;
    const int j = e == 2 ? 0 : e + 1, l = e == 0 ? 2 : e - 1;   // (e+1)%3, (e+2)%3
    if (i < 3) {
      la = 3 + l;
      lb = 3 + j;
    } else {
      la = k == 0 ? 3 + l : (k == 1 ? l : 3 + j);
      lb = k == 0 ? j : (k == 1 ? 3 + j : 3 + l);
    }
  }
}

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
  constexpr int NL = Elem<DEG>::NL;
  constexpr int NT = DEG == 1 ? 1 : 3;
  const int node = blockIdx.x * blockDim.x + threadIdx.x;
  if (node >= n) return;
  const int p0 = vptr[node], p1 = vptr[node + 1];
  // a row that leaves the map
  bool ok = p0 >= 0 && p1 >= p0 && p1 <= NL * nc;
  const double mine = old[node];
  double best = mine;
#pragma unroll 1
  for (int t = ok ? p0 : 0, te = ok ? p1 : 0; t < te; ++t) {
    const int s = vsrc[t];
    if (s < 0 || s >= NL * nc) {
      ok = false;
      continue;
    }
    const int i = s / nc, c = s - i * nc;
    const double x0 = xy[0 * nc + c], x1 = xy[1 * nc + c], x2 = xy[2 * nc + c];
    const double y0 = xy[3 * nc + c], y1 = xy[4 * nc + c], y2 = xy[5 * nc + c];
    const double cx = node_coord(i, x0, x1, x2), cy = node_coord(i, y0, y1, y2);
#pragma unroll
    for (int k = 0; k < NT; ++k) {
      if (k > 0 && i < 3) break;      // a vertex lies in one sub-triangle
      int la, lb;
      sub_triangle<DEG>(i, k, la, lb);
      const int da = cell_dofs[la * nc + c], db = cell_dofs[lb * nc + c];
      const bool in = da >= 0 && da < n && db >= 0 && db < n;
      ok = ok && in;
      const double ta = old[in ? da : 0], tb = old[in ? db : 0];
      const double cand =
          hopf_lax(cx, cy, node_coord(la, x0, x1, x2), node_coord(la, y0, y1, y2),
                   node_coord(lb, x0, x1, x2), node_coord(lb, y0, y1, y2), ta, tb);
      best = cand < best ? cand : best;
    }
  }
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
  FLOW_REQUIRE(mesh && mesh->nc >= 1 && mesh->nc <= INT_MAX / 6 && mesh->xy, "mesh");
  FLOW_REQUIRE(mesh->c1 == 0, "wall distance on strips");
  FLOW_REQUIRE(V && (V->deg == 1 || V->deg == 2) && V->n >= 1 && V->cell_dofs, "space");
  FLOW_REQUIRE(V->r1 == 0, "wall distance on strips");
  FLOW_REQUIRE(V->vptr && V->vsrc, "vector contribution map");
  FLOW_REQUIRE(nsweeps >= 1, "sweeps");
  FLOW_REQUIRE(buf_a && buf_b && flag, "pointers");
  FLOW_REQUIRE(buf_a != buf_b, "in place");
  hipStream_t st = as_stream(stream);
  const dim3 blocks((V->n + kBlock - 1) / kBlock);
  for (int k = 0; k < nsweeps; ++k) {
    const double* src = (k & 1) ? buf_b : buf_a;
    double* dst = (k & 1) ? buf_a : buf_b;
    // a sweep that lowers nothing has reached the fixed point, whatever the
    // sweeps before it did: only the last one of the batch reports
    int* f = k == nsweeps - 1 ? flag : nullptr;
    if (V->deg == 1)
      hipLaunchKernelGGL((distance_sweep_kernel<1>), blocks, dim3(kBlock), 0, st, mesh->nc,
                         mesh->xy, V->cell_dofs, V->n, V->vptr, V->vsrc, src, dst, f);
    else
      hipLaunchKernelGGL((distance_sweep_kernel<2>), blocks, dim3(kBlock), 0, st, mesh->nc,
                         mesh->xy, V->cell_dofs, V->n, V->vptr, V->vsrc, src, dst, f);
  }
  FLOW_CHECK_LAUNCH();
  return FLOW_OK;
}
