// The error indicator of the adaptive loop (flow_amd/fem/adapt.py):
//
//   flow_jump_indicator  eta2[T] = sum over the interior edges E of T of
//                        |E| / 24 * int_E sum_k [grad u_k . n]^2 ds, the jump
//                        of the normal derivative of a P1 / P2 field across
//                        the edges (Kelly et al.).  One lane per cell; every
//                        interior edge is evaluated from both of its cells, so
//                        a lane writes eta2[c] only: no atomics, no LDS, two
//                        calls give the same bits.  A lane holds its own
//                        geometry and dofs and ONE neighbour's at a time (the
//                        facet loop is not unrolled).  The neighbour is found
//                        through a packed per-facet table built on the host
//                        ([i*nc + c], adapt.facet_table): -1 on the boundary,
//                        else (cell << 3) | (its local facet << 1) | flip,
//                        flip = 0 when the FIRST vertex of the neighbour's
//                        facet is the first vertex of this cell's facet.  The
//                        point (1 - s) a + s b of this cell's edge is then the
//                        neighbour's barycentric (1 - s, s, 0) permuted: exact,
//                        no affine map is inverted.  Quadrature on the edge:
//                        P1 the mid point (the gradients are constant), P2 the
//                        2-point Gauss rule (the jump is linear along the edge,
//                        its square quadratic: exact).  Coalesced: the table,
//                        the lane's own geometry and dof indices, eta2;
//                        scattered (local where the cell numbering is): the
//                        neighbour's geometry and dof indices, all field values.
#include <cmath>

#include "fem_device.h"

namespace flow {
namespace {

// grad(lambda_k) . n of cell c, k = 0, 1, 2
__device__ __forceinline__ void normal_gradients(const Geom& g, double n0, double n1,
                                                 double gn[3]) {
#pragma unroll
  for (int k = 0; k < 3; ++k) gn[k] = g.gl[k][0] * n0 + g.gl[k][1] * n1;
}

template <int DEG, int NCOMP>
__global__ __launch_bounds__(kBlock) void jump_indicator_kernel(
    int nc, const double* __restrict__ xy, const int* __restrict__ cell_dofs, int n,
    const int* __restrict__ table, const double* __restrict__ u,
    double* __restrict__ eta2) {
  constexpr int NL = Elem<DEG>::NL;
  constexpr int NQ = DEG == 1 ? 1 : 2;
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nc) return;
  const Geom g = load_geom(xy, nc, c);
  bool ok = true;
  double U[NCOMP][NL];
#pragma unroll
  for (int l = 0; l < NL; ++l) {
    const int d = cell_dofs[l * nc + c];
    const bool in = d >= 0 && d < n;
    ok = ok && in;
#pragma unroll
    for (int a = 0; a < NCOMP; ++a)
      U[a][l] = in ? u[static_cast<size_t>(a) * n + d] : 0.0;
  }
  double total = 0.0;
#pragma unroll 1
  for (int i = 0; i < 3; ++i) {
    const int t = table[i * nc + c];
    if (t == -1) continue;                       // a boundary edge
    const int nb = t >> 3, j = (t >> 1) & 3, flip = t & 1;
    if (t < 0 || nb >= nc || j > 2) {
      ok = false;
      continue;
    }
    // (selects, not g.gl[i]: a run-time index would put g in scratch memory)
    const double gx = i == 0 ? g.gl[0][0] : (i == 1 ? g.gl[1][0] : g.gl[2][0]);
    const double gy = i == 0 ? g.gl[0][1] : (i == 1 ? g.gl[1][1] : g.gl[2][1]);
    const double gnorm = sqrt(gx * gx + gy * gy);
    const double n0 = -gx / gnorm, n1 = -gy / gnorm;
    const double len = g.adet * gnorm;
    double gn[3], hn[3];
    normal_gradients(g, n0, n1, gn);
    {
      const Geom h = load_geom(xy, nc, nb);
      normal_gradients(h, n0, n1, hn);
    }
    int dn[NL];
#pragma unroll
    for (int l = 0; l < NL; ++l) {
      const int d = cell_dofs[l * nc + nb];
      const bool in = d >= 0 && d < n;
      ok = ok && in;
      dn[l] = in ? d : 0;
    }
    double sum = 0.0;
#pragma unroll
    for (int a = 0; a < NCOMP; ++a) {
      double W[NL];
#pragma unroll
      for (int l = 0; l < NL; ++l) W[l] = u[static_cast<size_t>(a) * n + dn[l]];
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        const double s = DEG == 1 ? 0.5 : (q == 0 ? FLOW_G2A : FLOW_G2B);
        // this cell: facet i runs from vertex facet_v0(i) to facet_v1(i)
        const double L[3] = {i == 0 ? 0.0 : 1.0 - s,
                             i == 0 ? 1.0 - s : (i == 1 ? 0.0 : s),
                             i == 2 ? 0.0 : s};
        // the neighbour: the same point on its facet j
        const double p = flip ? s : 1.0 - s, r = 1.0 - p;
        const double M[3] = {j == 0 ? 0.0 : p, j == 0 ? p : (j == 1 ? 0.0 : r),
                             j == 2 ? 0.0 : r};
        double gu[3], gw[3];
        ref_gradient<DEG>(U[a], L, gu);
        ref_gradient<DEG>(W, M, gw);
        const double jump = (gu[0] * gn[0] + gu[1] * gn[1] + gu[2] * gn[2]) -
                            (gw[0] * hn[0] + gw[1] * hn[1] + gw[2] * hn[2]);
        sum += jump * jump;
      }
    }
    // int_E = |E| * mean over the rule's points
    total += (len / 24.0) * (len / NQ) * sum;
  }
  eta2[c] = ok ? total : __builtin_nan("");
}

}  // namespace
}  // namespace flow

using namespace flow;

extern "C" int flow_jump_indicator(const flow_mesh* mesh, const flow_space* V, int ncomp,
                                   const int* facet_table, const double* u,
                                   double* eta2, void* stream) {
  FLOW_REQUIRE(mesh && mesh->nc >= 1 && mesh->nc < (1 << 28) && mesh->xy, "mesh");
  FLOW_REQUIRE(mesh->c1 == 0, "jump indicator on strips");
  FLOW_REQUIRE(V && (V->deg == 1 || V->deg == 2) && V->n >= 1 && V->cell_dofs, "space");
  FLOW_REQUIRE(V->r1 == 0, "jump indicator on strips");
  FLOW_REQUIRE(ncomp == 1 || ncomp == 2, "components");
  FLOW_REQUIRE(facet_table && u && eta2, "pointers");
  FLOW_REQUIRE(u != eta2, "in place");
  hipStream_t st = as_stream(stream);
  const dim3 blocks((mesh->nc + kBlock - 1) / kBlock);
#define FLOW_JUMP(DEG, NCOMP)                                                       \
  hipLaunchKernelGGL((jump_indicator_kernel<DEG, NCOMP>), blocks, dim3(kBlock), 0, st, \
                     mesh->nc, mesh->xy, V->cell_dofs, V->n, facet_table, u, eta2)
  if (V->deg == 1) {
    if (ncomp == 1) FLOW_JUMP(1, 1);
    else FLOW_JUMP(1, 2);
  } else {
    if (ncomp == 1) FLOW_JUMP(2, 1);
    else FLOW_JUMP(2, 2);
  }
#undef FLOW_JUMP
  FLOW_CHECK_LAUNCH();
  return FLOW_OK;
}
