// The product of a Taylor-Hood matrix by blocks (flow_amd/fem/mixed.py,
// MixedMatrix) in ONE launch: flow_mixed_apply.  Unknowns are numbered velocity
// x, velocity y, pressure (2 nv + np doubles).
//
// MixedMatrix.apply composes the product of up to six flow_operator_apply
// launches, up to four axpby launches and a temporary: the velocity rows are
// written once and then read and written again per coupling plane.  Here a
// 256-thread workgroup owns one tile of rows and leaves every entry of y once:
//
//   velocity tile  rows [r0, r1) of BOTH components: the uu product through
//                  StreamTile2 (the four planes over the velocity pattern), then
//                  the two coupling planes up0, up1 over their shared
//                  RectLayout(kv, kp) pattern through StreamTilePlanes -- the
//                  column pairs and x_p loaded once for both --, y_u[r] = s_uu +
//                  s_up per component;
//   pressure tile  the pp row sum through StreamTile, then pu0 (gathers x[0:nv])
//                  and pu1 (gathers x[nv:2nv]) over their shared RectLayout(kp,
//                  kv) pattern, the column pairs loaded once, y_p = (s_pp +
//                  s_pu0) + s_pu1.
//
// A tile holds <= kBlock rows and no more nonzeros than the CSR-stream cap in
// EACH pattern it touches (the host builds the tiles: space.csr_stream_
// rowblocks over both row pointers).  All loads and gathers of a tile are issued
// before its first barrier; the two LDS planes (16 KB, what StreamTile2 needs)
// are reused between the phases of a tile behind a barrier.  No atomics.
//
// Bits: the tile structs are those of csr_stream.h, so a block's row sum is the
// sum of its parked products in ascending k, whatever the tiling -- the bits of
// flow_operator_apply for that block --, and axpby(1, t, 1, y) is one rounded
// addition (axpby_kernel: a x + b y with a = b = 1, fused or not).  A row sum is
// never -0.0 (it starts from +0.0), so 0.0 + s has the bits of s: an absent
// block may be skipped or added as 0.0 alike.  Every entry of y therefore has
// the bits MixedMatrix.apply leaves there, for every subset of present blocks.
//
// flow_mixed_upper_rhs is the first half of the block upper triangular
// preconditioner (mixed.py, BlockTriangularPreconditioner) over the same tiles,
// also in ONE launch: z_p = r_p * sinv and ru = r_u - up z_p.  The composed
// sequence is a vmul, a copy of r_u and, per coupling plane, a
// flow_operator_apply into a temporary and an axpby(-1, tmp, 1, ru): six
// launches, each plane streamed in a launch of its own.  Here
//
//   pressure tile  z_p[i] = r_p[i] * sinv[i];
//   velocity tile  the two planes up0, up1 through StreamTilePlanes, the column
//                  pairs loaded once; r_p and sinv are both gathered at the
//                  tile's columns and multiplied in the lane, so the operand
//                  z_p[col] never comes from memory and no velocity tile waits
//                  for a pressure tile; ru[c nv + i] = r[c nv + i] - s_c.
//
// Bits: vmul_kernel leaves 1.0 * r_p[i] * sinv[i], one rounded multiply, and
// the lane's r_p[col] * sinv[col] is the same multiply of the same operands, so
// the parked products are those of flow_operator_apply on the stored z_p; the
// row sum is the tile structs' sum in ascending k; axpby(-1, tmp, 1, ru) is
// -1 * tmp + 1 * ru, whose two products are exact, fused or not: one rounded
// subtraction ru - tmp.  A component whose plane is absent keeps the bits of
// r (the copy).  Every entry of z_p and ru therefore has the bits the composed
// sequence leaves, for every subset of present planes.  No atomics, and no LDS
// beyond the two planes declared for the product.
#include "csr_stream.h"
#include "multi_dot.h"

namespace flow {
namespace {

constexpr int kTileM = kTile > kTile2 ? kTile : kTile2;   // doubles per LDS plane

__device__ __forceinline__ void mixed_velocity_tile(
    const flow_mixed& A, int r0, int r1, const double* __restrict__ x,
    double* __restrict__ y, double* __restrict__ prod0, double* __restrict__ prod1) {
  const int nv = A.nv;
  const int r = r0 + threadIdx.x;
  // (block-uniform)
  const bool uu = A.uu[0] != nullptr;
  const bool up0 = A.up[0] != nullptr, up1 = A.up[1] != nullptr;
  StreamTile2 t;
  StreamTilePlanes c;
  StreamTile2::Gathered gu;
  StreamTile::Gathered gp;
  if (uu) t.load(r0, r1, A.vrowptr, A.vcols, A.uu[0], A.uu[1], A.uu[2], A.uu[3]);
  if (up0 || up1)   // (an absent plane: the other's values, loaded and unused)
    c.load(r0, r1, A.uprowptr, A.upcols, up0 ? A.up[0] : A.up[1],
           up1 ? A.up[1] : A.up[0]);
  if (uu) gu = t.gather(x, nv);
  if (up0 || up1) gp = c.gather(A.upcols, x + 2 * static_cast<size_t>(nv));
  double s0 = 0.0, s1 = 0.0;
  if (uu) {
    t.park(gu, prod0, prod1);
    __syncthreads();
    const double2 s = t.sum(prod0, prod1);
    s0 = s.x;
    s1 = s.y;
  }
  if (up0 || up1) {
    if (uu) __syncthreads();   // the planes have been summed
    if (up0) c.plane(0).park(gp, prod0);
    if (up1) c.plane(1).park(gp, prod1);
    __syncthreads();
    if (up0) s0 += c.sum(prod0);
    if (up1) s1 += c.sum(prod1);
  }
  if (r < r1) {
    y[r] = s0;
    y[nv + r] = s1;
  }
}

__device__ __forceinline__ void mixed_pressure_tile(
    const flow_mixed& A, int r0, int r1, const double* __restrict__ x,
    double* __restrict__ y, double* __restrict__ prod0, double* __restrict__ prod1) {
  const int nv = A.nv;
  const int r = r0 + threadIdx.x;
  // (block-uniform)
  const bool pp = A.pp != nullptr;
  const bool pu0 = A.pu[0] != nullptr, pu1 = A.pu[1] != nullptr;
  StreamTile t;
  StreamTilePlanes c;
  StreamTile::Gathered gp, g0, g1;
  if (pp) t.load(r0, r1, A.prowptr, A.pcols, A.pp);
  if (pu0 || pu1)
    c.load(r0, r1, A.purowptr, A.pucols, pu0 ? A.pu[0] : A.pu[1],
           pu1 ? A.pu[1] : A.pu[0]);
  if (pp) gp = t.gather(A.pcols, x + 2 * static_cast<size_t>(nv));
  if (pu0) g0 = c.gather(A.pucols, x);
  if (pu1) g1 = c.gather(A.pucols, x + nv);
  double s = 0.0;
  if (pp) {
    t.park(gp, prod0);
    __syncthreads();
    s = t.sum(prod0);
  }
  if (pu0 || pu1) {
    if (pp) __syncthreads();   // the plane has been summed
    if (pu0) c.plane(0).park(g0, prod0);
    if (pu1) c.plane(1).park(g1, prod1);
    __syncthreads();
    if (pu0) s += c.sum(prod0);
    if (pu1) s += c.sum(prod1);
  }
  if (r < r1) y[2 * static_cast<size_t>(nv) + r] = s;
}

__global__ __launch_bounds__(kBlock) void mixed_apply_kernel(
    flow_mixed A, const double* __restrict__ x, double* __restrict__ y) {
  __shared__ double prod0[kTileM];
  __shared__ double prod1[kTileM];
  const int tile = xcd_tile(blockIdx.x, gridDim.x);
  if (tile < A.nvtiles) {
    mixed_velocity_tile(A, A.vtiles[tile], A.vtiles[tile + 1], x, y, prod0, prod1);
  } else {
    const int pt = tile - A.nvtiles;
    mixed_pressure_tile(A, A.ptiles[pt], A.ptiles[pt + 1], x, y, prod0, prod1);
  }
}
static_assert(2 * kTileM * sizeof(double) <= 32768,
              "two LDS planes (16 KB with two pairs per lane)");

__device__ __forceinline__ void upper_rhs_velocity_tile(
    const flow_mixed& A, int r0, int r1, const double* __restrict__ sinv,
    const double* __restrict__ r, double* __restrict__ ru,
    double* __restrict__ prod0, double* __restrict__ prod1) {
  const int nv = A.nv;
  const int row = r0 + threadIdx.x;
  // (block-uniform)
  const bool up0 = A.up[0] != nullptr, up1 = A.up[1] != nullptr;
  StreamTilePlanes c;
  StreamTile::Gathered g, gs;
  if (up0 || up1)   // (an absent plane: the other's values, loaded and unused)
    c.load(r0, r1, A.uprowptr, A.upcols, up0 ? A.up[0] : A.up[1],
           up1 ? A.up[1] : A.up[0]);
  double b0 = 0.0, b1 = 0.0;
  if (row < r1) {
    b0 = r[row];
    b1 = r[nv + row];
  }
  if (up0 || up1) {
    g = c.gather(A.upcols, r + 2 * static_cast<size_t>(nv));
    gs = c.gather(A.upcols, sinv);
#pragma unroll
    for (int j = 0; j < kPairs; ++j) {   // z_p at the columns: vmul's multiply
      g.x0[j] = g.x0[j] * gs.x0[j];
      g.x1[j] = g.x1[j] * gs.x1[j];
    }
    if (up0) c.plane(0).park(g, prod0);
    if (up1) c.plane(1).park(g, prod1);
    __syncthreads();
    if (up0) b0 = b0 - c.sum(prod0);
    if (up1) b1 = b1 - c.sum(prod1);
  }
  if (row < r1) {
    ru[row] = b0;
    ru[nv + row] = b1;
  }
}

__global__ __launch_bounds__(kBlock) void mixed_upper_rhs_kernel(
    flow_mixed A, const double* __restrict__ sinv, const double* __restrict__ r,
    double* __restrict__ z_p, double* __restrict__ ru) {
  __shared__ double prod0[kTileM];
  __shared__ double prod1[kTileM];
  const int tile = xcd_tile(blockIdx.x, gridDim.x);
  if (tile < A.nvtiles) {
    upper_rhs_velocity_tile(A, A.vtiles[tile], A.vtiles[tile + 1], sinv, r, ru,
                            prod0, prod1);
  } else {
    const int pt = tile - A.nvtiles;
    const int i = A.ptiles[pt] + threadIdx.x;
    if (i < A.ptiles[pt + 1])
      z_p[i] = 1.0 * r[2 * static_cast<size_t>(A.nv) + i] * sinv[i];
  }
}

bool plane_ok(const double* p) { return p == nullptr || aligned16(p); }

}  // namespace
}  // namespace flow

using namespace flow;

extern "C" int flow_mixed_apply(const flow_mixed* A, const double* x, double* y,
                                void* stream) {
  FLOW_REQUIRE(A != nullptr, "mixed operator is NULL");
  FLOW_REQUIRE(A->nv > 0 && A->np > 0, "mixed operator sizes");
  FLOW_REQUIRE(A->nvtiles > 0 && A->nptiles > 0 && A->vtiles && A->ptiles,
               "mixed operator tiles");
  const bool uu = A->uu[0] != nullptr;
  FLOW_REQUIRE((A->uu[1] != nullptr) == uu && (A->uu[2] != nullptr) == uu &&
                   (A->uu[3] != nullptr) == uu,
               "mixed operator: the four uu planes are present or absent together");
  FLOW_REQUIRE(!uu || (A->vrowptr && A->vcols), "mixed operator: velocity pattern");
  FLOW_REQUIRE(!(A->up[0] || A->up[1]) || (A->uprowptr && A->upcols),
               "mixed operator: up pattern");
  FLOW_REQUIRE(!A->pp || (A->prowptr && A->pcols), "mixed operator: pressure pattern");
  FLOW_REQUIRE(!(A->pu[0] || A->pu[1]) || (A->purowptr && A->pucols),
               "mixed operator: pu pattern");
  FLOW_REQUIRE(plane_ok(A->uu[0]) && plane_ok(A->uu[1]) && plane_ok(A->uu[2]) &&
                   plane_ok(A->uu[3]) && plane_ok(A->up[0]) && plane_ok(A->up[1]) &&
                   plane_ok(A->pp) && plane_ok(A->pu[0]) && plane_ok(A->pu[1]),
               "value planes must be 16-byte aligned");
  const auto cols_ok = [](const int* c) {
    return (reinterpret_cast<size_t>(c) & 7) == 0;
  };
  FLOW_REQUIRE(cols_ok(A->vcols) && cols_ok(A->upcols) && cols_ok(A->pcols) &&
                   cols_ok(A->pucols),
               "cols must be 8-byte aligned");
  FLOW_REQUIRE(x && y, "mixed product pointers");
  const size_t n = 2 * static_cast<size_t>(A->nv) + static_cast<size_t>(A->np);
  FLOW_REQUIRE(!overlap(y, n, x, n), "mixed product: y overlaps x");
  hipLaunchKernelGGL(mixed_apply_kernel, dim3(A->nvtiles + A->nptiles), dim3(kBlock),
                     0, as_stream(stream), *A, x, y);
  FLOW_CHECK_LAUNCH();
  return FLOW_OK;
}

extern "C" int flow_mixed_upper_rhs(const flow_mixed* A, const double* sinv,
                                    const double* r, double* z_p, double* ru,
                                    void* stream) {
  FLOW_REQUIRE(A != nullptr, "mixed operator is NULL");
  FLOW_REQUIRE(A->nv > 0 && A->np > 0, "mixed operator sizes");
  FLOW_REQUIRE(A->nvtiles > 0 && A->nptiles > 0 && A->vtiles && A->ptiles,
               "mixed operator tiles");
  FLOW_REQUIRE(!(A->up[0] || A->up[1]) || (A->uprowptr && A->upcols),
               "mixed operator: up pattern");
  FLOW_REQUIRE(plane_ok(A->up[0]) && plane_ok(A->up[1]),
               "value planes must be 16-byte aligned");
  FLOW_REQUIRE((reinterpret_cast<size_t>(A->upcols) & 7) == 0,
               "cols must be 8-byte aligned");
  FLOW_REQUIRE(sinv && r && z_p && ru, "mixed upper rhs pointers");
  const size_t n2 = 2 * static_cast<size_t>(A->nv);
  const size_t np = static_cast<size_t>(A->np);
  FLOW_REQUIRE(!overlap(ru, n2, r, n2 + np), "mixed upper rhs: ru overlaps r");
  FLOW_REQUIRE(!overlap(z_p, np, r, n2 + np), "mixed upper rhs: z_p overlaps r");
  FLOW_REQUIRE(!overlap(ru, n2, sinv, np) && !overlap(z_p, np, sinv, np),
               "mixed upper rhs: an output overlaps sinv");
  FLOW_REQUIRE(!overlap(ru, n2, z_p, np), "mixed upper rhs: ru overlaps z_p");
  hipLaunchKernelGGL(mixed_upper_rhs_kernel, dim3(A->nvtiles + A->nptiles),
                     dim3(kBlock), 0, as_stream(stream), *A, sinv, r, z_p, ru);
  FLOW_CHECK_LAUNCH();
  return FLOW_OK;
}
