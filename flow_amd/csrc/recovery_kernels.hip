// Recovered nodal gradients and the ZZ error indicator (flow_amd/fem/
// recovery.py): the two kernels behind fem.GradientRecovery.
//
//   flow_recover_gradient  G_k(n) = sum_c |T_c| grad u_k|_c(x_n) / sum_c |T_c|
//                          over the cells c of the patch of node n: the
//                          area-weighted mean of the cell gradients AT the node
//                          (Zienkiewicz-Zhu).  One lane per node of the scalar
//                          layout, all components; the patch is the node's row
//                          of the vector contribution map (vptr / vsrc, entry
//                          i*nc + c: local node i of cell c), walked in the
//                          map's order: no atomics, no LDS, two calls give the
//                          same bits.  Local nodes 0-2 are the vertices, 3-5
//                          the mid points of the edges opposite them; the
//                          barycentric point is built with selects, the basis
//                          gradients by basis<DEG> / phys_grad.  The sums of
//                          one component are explicit fma chains that do not
//                          depend on NCOMP: a component of a vector field gets
//                          the bits the scalar call gives it.  Coalesced: vptr,
//                          out; streamed per lane: its row of vsrc; scattered
//                          (local where the numbering follows the mesh): the
//                          patch cells' coordinates, dof indices and values.
//   flow_zz_indicator      eta2[c] = sum_k int_T |G_k - grad u_k|^2 dx, G_k
//                          interpolated in P_deg, by the rule handed in (rows
//                          (xi, eta, w), weights summing to 1/2: the convention
//                          of form_kernels.hip).  One lane per cell; the
//                          cell's dofs, u and G values stay in registers (the
//                          loop over the rule's points is the only run-time
//                          loop and indexes the rule alone).
#include <climits>
#include <cmath>

#include "fem_device.h"

namespace flow {
namespace {

// one lane per node
template <int DEG, int NCOMP>
__global__ __launch_bounds__(kBlock) void recover_gradient_kernel(
    int nc, const double* __restrict__ xy, const int* __restrict__ cell_dofs, int n,
    const int* __restrict__ vptr, const int* __restrict__ vsrc,
    const double* __restrict__ u, double* __restrict__ out) {
  constexpr int NL = Elem<DEG>::NL;
  const int node = blockIdx.x * blockDim.x + threadIdx.x;
  if (node >= n) return;
  const int p0 = vptr[node], p1 = vptr[node + 1];
  // an empty patch, or a row that leaves the map
  bool ok = p0 >= 0 && p1 > p0 && p1 <= NL * nc;
  double acc[NCOMP][2];
#pragma unroll
  for (int a = 0; a < NCOMP; ++a) acc[a][0] = acc[a][1] = 0.0;
  double wsum = 0.0;
#pragma unroll 1
  for (int t = ok ? p0 : 0, te = ok ? p1 : 0; t < te; ++t) {
    const int s = vsrc[t];
    if (s < 0 || s >= NL * nc) {
      ok = false;
      continue;
    }
    const int i = s / nc, c = s - i * nc;
    const Geom g = load_geom(xy, nc, c);
    int d[NL];
#pragma unroll
    for (int l = 0; l < NL; ++l) {
      const int dl = cell_dofs[l * nc + c];
      const bool in = dl >= 0 && dl < n;
      ok = ok && in;
      d[l] = in ? dl : 0;
    }
    // the reference position of local node i (selects: no run-time index)
    const double L[3] = {
        i < 3 ? (i == 0 ? 1.0 : 0.0) : (i == 3 ? 0.0 : 0.5),
        i < 3 ? (i == 1 ? 1.0 : 0.0) : (i == 4 ? 0.0 : 0.5),
        i < 3 ? (i == 2 ? 1.0 : 0.0) : (i == 5 ? 0.0 : 0.5)};
    double phi[NL], dphi[NL][3], gphi[NL][2];
    basis<DEG>(L, phi, dphi);
    phys_grad<NL>(g, dphi, gphi);
    const double area = 0.5 * g.adet;
    wsum += area;
#pragma unroll
    for (int a = 0; a < NCOMP; ++a) {
      const double* __restrict__ ua = u + static_cast<size_t>(a) * n;
      double gx = 0.0, gy = 0.0;
#pragma unroll
      for (int l = 0; l < NL; ++l) {
        const double ul = ua[d[l]];
        gx = fma(ul, gphi[l][0], gx);
        gy = fma(ul, gphi[l][1], gy);
      }
      acc[a][0] = fma(area, gx, acc[a][0]);
      acc[a][1] = fma(area, gy, acc[a][1]);
    }
  }
#pragma unroll
  for (int a = 0; a < NCOMP; ++a) {
#pragma unroll
    for (int k = 0; k < 2; ++k)
      out[static_cast<size_t>(2 * a + k) * n + node] =
          ok ? acc[a][k] / wsum : __builtin_nan("");
  }
}

// one lane per cell
template <int DEG, int NCOMP>
__global__ __launch_bounds__(kBlock) void zz_indicator_kernel(
    int nc, const double* __restrict__ xy, const int* __restrict__ cell_dofs, int n,
    const double* __restrict__ u, const double* __restrict__ G, int nq,
    const double* __restrict__ rule, double* __restrict__ eta2) {
  constexpr int NL = Elem<DEG>::NL;
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nc) return;
  const Geom g = load_geom(xy, nc, c);
  bool ok = true;
  double U[NCOMP][NL], R[NCOMP][2][NL];
#pragma unroll
  for (int l = 0; l < NL; ++l) {
    const int dl = cell_dofs[l * nc + c];
    const bool in = dl >= 0 && dl < n;
    ok = ok && in;
    const int d = in ? dl : 0;
#pragma unroll
    for (int a = 0; a < NCOMP; ++a) {
      U[a][l] = u[static_cast<size_t>(a) * n + d];
      R[a][0][l] = G[static_cast<size_t>(2 * a) * n + d];
      R[a][1][l] = G[static_cast<size_t>(2 * a + 1) * n + d];
    }
  }
  double total = 0.0;
#pragma unroll 1
  for (int q = 0; q < nq; ++q) {
    const double xi = rule[3 * q], eta = rule[3 * q + 1];
    const double w = rule[3 * q + 2] * g.adet;
    const double L[3] = {1.0 - xi - eta, xi, eta};
    double phi[NL], dphi[NL][3], gphi[NL][2];
    basis<DEG>(L, phi, dphi);
    phys_grad<NL>(g, dphi, gphi);
    double sum = 0.0;
#pragma unroll
    for (int a = 0; a < NCOMP; ++a) {
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        double diff = 0.0;
#pragma unroll
        for (int l = 0; l < NL; ++l)
          diff += R[a][k][l] * phi[l] - U[a][l] * gphi[l][k];
        sum += diff * diff;
      }
    }
    total += w * sum;
  }
  eta2[c] = ok ? total : __builtin_nan("");
}

int check_operands(const flow_mesh* mesh, const flow_space* V, int ncomp) {
  FLOW_REQUIRE(mesh && mesh->nc >= 1 && mesh->nc <= INT_MAX / 6 && mesh->xy, "mesh");
  FLOW_REQUIRE(mesh->c1 == 0, "gradient recovery on strips");
  FLOW_REQUIRE(V && (V->deg == 1 || V->deg == 2) && V->n >= 1 && V->cell_dofs, "space");
  FLOW_REQUIRE(V->r1 == 0, "gradient recovery on strips");
  FLOW_REQUIRE(ncomp == 1 || ncomp == 2, "components");
  return FLOW_OK;
}

}  // namespace
}  // namespace flow

using namespace flow;

extern "C" int flow_recover_gradient(const flow_mesh* mesh, const flow_space* V, int ncomp,
                                     const double* u, double* out, void* stream) {
  const int rc = check_operands(mesh, V, ncomp);
  if (rc) return rc;
  FLOW_REQUIRE(V->vptr && V->vsrc, "vector contribution map");
  FLOW_REQUIRE(u && out, "pointers");
  FLOW_REQUIRE(u != out, "in place");
  hipStream_t st = as_stream(stream);
  const dim3 blocks((V->n + kBlock - 1) / kBlock);
#define FLOW_RECOVER(DEG, NCOMP)                                                       \
  hipLaunchKernelGGL((recover_gradient_kernel<DEG, NCOMP>), blocks, dim3(kBlock), 0, st, \
                     mesh->nc, mesh->xy, V->cell_dofs, V->n, V->vptr, V->vsrc, u, out)
  if (V->deg == 1) {
    if (ncomp == 1) FLOW_RECOVER(1, 1);
    else FLOW_RECOVER(1, 2);
  } else {
    if (ncomp == 1) FLOW_RECOVER(2, 1);
    else FLOW_RECOVER(2, 2);
  }
#undef FLOW_RECOVER
  FLOW_CHECK_LAUNCH();
  return FLOW_OK;
}

extern "C" int flow_zz_indicator(const flow_mesh* mesh, const flow_space* V, int ncomp,
                                 const double* u, const double* G, int nq,
                                 const double* rule, double* eta2, void* stream) {
  const int rc = check_operands(mesh, V, ncomp);
  if (rc) return rc;
  FLOW_REQUIRE(nq >= 1 && nq <= FLOW_FORM_MAX_POINTS && rule, "quadrature rule");
  FLOW_REQUIRE(u && G && eta2, "pointers");
  FLOW_REQUIRE(u != eta2 && G != eta2, "in place");
  hipStream_t st = as_stream(stream);
  const dim3 blocks((mesh->nc + kBlock - 1) / kBlock);
#define FLOW_ZZ(DEG, NCOMP)                                                        \
  hipLaunchKernelGGL((zz_indicator_kernel<DEG, NCOMP>), blocks, dim3(kBlock), 0, st, \
                     mesh->nc, mesh->xy, V->cell_dofs, V->n, u, G, nq, rule, eta2)
  if (V->deg == 1) {
    if (ncomp == 1) FLOW_ZZ(1, 1);
    else FLOW_ZZ(1, 2);
  } else {
    if (ncomp == 1) FLOW_ZZ(2, 1);
    else FLOW_ZZ(2, 2);
  }
#undef FLOW_ZZ
  FLOW_CHECK_LAUNCH();
  return FLOW_OK;
}
