// Contour lines and level-set measures of a nodal field (flow_amd/fem/
// isolines.py): the kernels behind fem.Isolines.
//
// The field is f_h, the continuous piecewise-LINEAR interpolant of the nodal
// values: on P1 the field itself, on P2 every cell cut into its three corner
// triangles (v_i, e_(i+2), e_(i+1)) and the middle one (e_0, e_1, e_2), local
// dofs [v0 v1 v2 e0 e1 e2] with e_i opposite v_i -- the sub-triangulation of
// distance_kernels.hip, in this order.
//
//   flow_isoline_count    one lane per cell: the cell's dofs (SoA, coalesced),
//                         the gather of f, then per level of the launch the
//                         number of segments of the cell; count[cell].
//   flow_isoline_emit     the same lanes; a cell with a non-zero count loads
//                         its geometry and writes its segments behind
//                         offset[cell]: by level, then by sub-triangle.
//   flow_isoline_measure  the same lanes; per level the length of the cell's
//                         segments and the area of {f_h >= c} in the cell,
//                         block sums to partials[2*level + q][block], and a
//                         second launch that adds the partials in block order.
//
// Definitions (all three agree; tests/isolines_reference.py restates them).
// A node is ABOVE iff f >= c.  A sub-triangle whose three values are finite
// and not all on one side holds one segment, between the crossings of the two
// sub-edges that join the node that is alone on its side to the other two --
// unless that node is above and lies exactly on the level: both crossings are
// then the node itself and nothing is emitted.  The crossing of the sub-edge
// with global dofs a < b is x_a + t (x_b - x_a), t = (c - f_a) / (f_b - f_a),
// always from the lower dof to the higher and without contraction, so that the
// two cells at an edge compute the same bits (the mid points 0.5 (v_j + v_k)
// are the same bits in both cells, too: the sum commutes).  The segment has
// the above side on its left.
//
// No atomics, no LDS but the block sums, no private memory: the sub-triangles
// are unrolled, so their local nodes are constants, and the node that is alone
// is turned into values by selects (as form_facet does for the facet's
// vertices).  The levels travel in the kernel arguments.
#include <climits>
#include <cmath>

#include "fem_device.h"

namespace flow {
namespace {

constexpr int kMaxLev = FLOW_ISOLINE_LEVELS_PER_LAUNCH;

struct Node {
  int d;             // global dof
  double f, x, y;    // value, position
  double l0, l1, l2; // barycentric coordinates in the parent cell
};

__device__ __forceinline__ Node pick(int p, const Node& a, const Node& b, const Node& c) {
  Node r;
  r.d = p == 0 ? a.d : (p == 1 ? b.d : c.d);
  r.f = p == 0 ? a.f : (p == 1 ? b.f : c.f);
  r.x = p == 0 ? a.x : (p == 1 ? b.x : c.x);
  r.y = p == 0 ? a.y : (p == 1 ? b.y : c.y);
  r.l0 = p == 0 ? a.l0 : (p == 1 ? b.l0 : c.l0);
  r.l1 = p == 0 ? a.l1 : (p == 1 ? b.l1 : c.l1);
  r.l2 = p == 0 ? a.l2 : (p == 1 ? b.l2 : c.l2);
  return r;
}

struct Crossing {
  int a, b;          // the sub-edge, a < b
  double x, y, l0, l1, l2;
};

// the crossing of the sub-edge between u and v, from the lower dof
__device__ __forceinline__ Crossing cross(const Node& u, const Node& v, double c) {
#pragma clang fp contract(off)
  const bool lo = u.d < v.d;
  const double fa = lo ? u.f : v.f, fb = lo ? v.f : u.f;
  const double xa = lo ? u.x : v.x, xb = lo ? v.x : u.x;
  const double ya = lo ? u.y : v.y, yb = lo ? v.y : u.y;
  const double t = (c - fa) / (fb - fa);
  Crossing r;
  r.a = lo ? u.d : v.d;
  r.b = lo ? v.d : u.d;
  r.x = xa + t * (xb - xa);
  r.y = ya + t * (yb - ya);
  const double a0 = lo ? u.l0 : v.l0, b0 = lo ? v.l0 : u.l0;
  const double a1 = lo ? u.l1 : v.l1, b1 = lo ? v.l1 : u.l1;
  const double a2 = lo ? u.l2 : v.l2, b2 = lo ? v.l2 : u.l2;
  r.l0 = a0 + t * (b0 - a0);
  r.l1 = a1 + t * (b1 - a1);
  r.l2 = a2 + t * (b2 - a2);
  return r;
}

__device__ __forceinline__ bool finite3(double a, double b, double c) {
  return fabs(a) < __builtin_inf() && fabs(b) < __builtin_inf() &&
         fabs(c) < __builtin_inf();
}

// does the sub-triangle with these values hold a segment of level c?
__device__ __forceinline__ bool crossed(double f0, double f1, double f2, double c) {
  const int na = (f0 >= c) + (f1 >= c) + (f2 >= c);
  const bool tie = f0 == c || f1 == c || f2 == c;   // (a node below is not on c)
  return finite3(f0, f1, f2) && (na == 2 || (na == 1 && !tie));
}

// the values of a cell: dofs in range (else 0 is read and ok is false)
template <int DEG>
struct CellValues {
  int d[Elem<DEG>::NL];
  double f[Elem<DEG>::NL];
  double lo, hi;     // over the values that are not NaN
  bool ok;
};

template <int DEG>
__device__ __forceinline__ CellValues<DEG> load_values(int nc, int c, int n,
                                                        const int* __restrict__ cell_dofs,
                                                        const double* __restrict__ f) {
  constexpr int NL = Elem<DEG>::NL;
  CellValues<DEG> v;
  v.ok = true;
#pragma unroll
  for (int l = 0; l < NL; ++l) {
    v.d[l] = cell_dofs[l * nc + c];
    const bool in = v.d[l] >= 0 && v.d[l] < n;
    v.ok = v.ok && in;
    v.f[l] = f[in ? v.d[l] : 0];
  }
  v.lo = v.f[0];
  v.hi = v.f[0];
#pragma unroll
  for (int l = 1; l < NL; ++l) {
    v.lo = fmin(v.lo, v.f[l]);
    v.hi = fmax(v.hi, v.f[l]);
  }
  return v;
}

// local nodes of sub-triangle s (compile-time after unrolling)
template <int DEG>
__device__ __forceinline__ constexpr int sub_node(int s, int k) {
  if (DEG == 1) return k;
  if (s == 3) return 3 + k;
  // corner s: (v_s, e_(s+2), e_(s+1))
  return k == 0 ? s : (k == 1 ? 3 + (s + 2) % 3 : 3 + (s + 1) % 3);
}

template <int DEG>
struct CellNodes {
  Node n[Elem<DEG>::NL];
  bool cw;           // the cell is clockwise
  double sub_area;   // area of one sub-triangle
};

template <int DEG>
__device__ __forceinline__ CellNodes<DEG> load_nodes(const double* __restrict__ xy, int nc,
                                                      int c, const CellValues<DEG>& v) {
#pragma clang fp contract(off)
  constexpr int NL = Elem<DEG>::NL;
  const double x0 = xy[0 * nc + c], x1 = xy[1 * nc + c], x2 = xy[2 * nc + c];
  const double y0 = xy[3 * nc + c], y1 = xy[4 * nc + c], y2 = xy[5 * nc + c];
  CellNodes<DEG> g;
  const double det = (x1 - x0) * (y2 - y0) - (x2 - x0) * (y1 - y0);
  g.cw = det < 0.0;
  g.sub_area = (DEG == 1 ? 0.5 : 0.125) * fabs(det);
  g.n[0] = Node{v.d[0], v.f[0], x0, y0, 1.0, 0.0, 0.0};
  g.n[1] = Node{v.d[1], v.f[1], x1, y1, 0.0, 1.0, 0.0};
  g.n[2] = Node{v.d[2], v.f[2], x2, y2, 0.0, 0.0, 1.0};
  if constexpr (NL == 6) {
    g.n[3] = Node{v.d[3], v.f[3], 0.5 * (x1 + x2), 0.5 * (y1 + y2), 0.0, 0.5, 0.5};
    g.n[4] = Node{v.d[4], v.f[4], 0.5 * (x0 + x2), 0.5 * (y0 + y2), 0.5, 0.0, 0.5};
    g.n[5] = Node{v.d[5], v.f[5], 0.5 * (x0 + x1), 0.5 * (y0 + y1), 0.5, 0.5, 0.0};
  }
  return g;
}

// the segment of a crossed sub-triangle (A, B, C in the cell's cyclic order):
// from `from` to `to`, the above side on the left
__device__ __forceinline__ void segment(const Node& A, const Node& B, const Node& C,
                                        double c, bool cw, Crossing& from, Crossing& to) {
  const bool a0 = A.f >= c, a1 = B.f >= c, a2 = C.f >= c;
  const bool one = (a0 + a1 + a2) == 1;       // the node alone is the one above
  // the node alone on its side, and the two behind it in cyclic order
  const int p = one ? (a0 ? 0 : (a1 ? 1 : 2)) : (!a0 ? 0 : (!a1 ? 1 : 2));
  const Node P = pick(p, A, B, C), Q = pick(p, B, C, A), R = pick(p, C, A, B);
  const Crossing pq = cross(P, Q, c), pr = cross(P, R, c);
  // counter-clockwise and P above: from P-Q to P-R keeps P on the left
  const bool swap = one == cw;
  from = swap ? pr : pq;
  to = swap ? pq : pr;
}

// ---- count -------------------------------------------------------------------
template <int DEG>
__global__ __launch_bounds__(kBlock) void isoline_count_kernel(
    int nc, const int* __restrict__ cell_dofs, int n, const double* __restrict__ f,
    const flow_isoline_levels L, int* __restrict__ count) {
  constexpr int NS = DEG == 1 ? 1 : 4;
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nc) return;
  const CellValues<DEG> v = load_values<DEG>(nc, c, n, cell_dofs, f);
  int total = 0;
#pragma unroll 1
  for (int l = 0; l < L.n; ++l) {
    const double lev = L.c[l];
    if (!(v.lo < lev && lev <= v.hi)) continue;
#pragma unroll
    for (int s = 0; s < NS; ++s)
      total += crossed(v.f[sub_node<DEG>(s, 0)], v.f[sub_node<DEG>(s, 1)],
                       v.f[sub_node<DEG>(s, 2)], lev);
  }
  // a cell that names a dof outside [0, n): one record, filled with NaN and -1
  count[c] = v.ok ? total : 1;
}

// ---- emit --------------------------------------------------------------------
template <int DEG>
__global__ __launch_bounds__(kBlock) void isoline_emit_kernel(
    int nc, const double* __restrict__ xy, const int* __restrict__ cell_dofs, int n,
    const double* __restrict__ f, const flow_isoline_levels L,
    const int* __restrict__ count, const int* __restrict__ offset, int capacity,
    double* __restrict__ seg_xy, int* __restrict__ seg_level, int* __restrict__ seg_cell,
    int* __restrict__ seg_keys, double* __restrict__ seg_bary) {
  constexpr int NS = DEG == 1 ? 1 : 4;
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nc) return;
  const int cnt = count[c];
  if (cnt <= 0) return;
  const int first = offset[c];
  if (first < 0 || first >= capacity) return;
  const CellValues<DEG> v = load_values<DEG>(nc, c, n, cell_dofs, f);
  if (!v.ok) {
    const double nan = __builtin_nan("");
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      seg_xy[4 * (size_t)first + k] = nan;
      seg_keys[4 * (size_t)first + k] = -1;
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) seg_bary[6 * (size_t)first + k] = nan;
    seg_level[first] = -1;
    seg_cell[first] = c;
    return;
  }
  const CellNodes<DEG> g = load_nodes<DEG>(xy, nc, c, v);
  int k = 0;         // segments of this cell so far: never more than count[c]
#pragma unroll 1
  for (int l = 0; l < L.n; ++l) {
    const double lev = L.c[l];
    if (!(v.lo < lev && lev <= v.hi)) continue;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const Node& A = g.n[sub_node<DEG>(s, 0)];
      const Node& B = g.n[sub_node<DEG>(s, 1)];
      const Node& C = g.n[sub_node<DEG>(s, 2)];
      if (!crossed(A.f, B.f, C.f, lev)) continue;
      const long long at = (long long)first + k;
      if (k < cnt && at < capacity) {
        Crossing p, q;
        segment(A, B, C, lev, g.cw, p, q);
        const size_t i = (size_t)at;
        seg_xy[4 * i + 0] = p.x;
        seg_xy[4 * i + 1] = p.y;
        seg_xy[4 * i + 2] = q.x;
        seg_xy[4 * i + 3] = q.y;
        seg_keys[4 * i + 0] = p.a;
        seg_keys[4 * i + 1] = p.b;
        seg_keys[4 * i + 2] = q.a;
        seg_keys[4 * i + 3] = q.b;
        seg_bary[6 * i + 0] = p.l0;
        seg_bary[6 * i + 1] = p.l1;
        seg_bary[6 * i + 2] = p.l2;
        seg_bary[6 * i + 3] = q.l0;
        seg_bary[6 * i + 4] = q.l1;
        seg_bary[6 * i + 5] = q.l2;
        seg_level[i] = L.base + l;
        seg_cell[i] = c;
      }
      ++k;
    }
  }
}

// ---- measure -----------------------------------------------------------------
// area of {f_h >= c} in a sub-triangle of area `area` with finite values: with
// P the node alone on its side, the corner cut off at P is the share s_pq s_pr
// of the triangle, s_pk = (c - f_P) / (f_k - f_P) the way from P to the crossing
__device__ __forceinline__ double area_above(double f0, double f1, double f2, double c,
                                             double area) {
  const bool a0 = f0 >= c, a1 = f1 >= c, a2 = f2 >= c;
  const int na = a0 + a1 + a2;
  if (na == 0) return 0.0;
  if (na == 3) return area;
  const bool one = na == 1;
  const int p = one ? (a0 ? 0 : (a1 ? 1 : 2)) : (!a0 ? 0 : (!a1 ? 1 : 2));
  const double fp = p == 0 ? f0 : (p == 1 ? f1 : f2);
  const double fq = p == 0 ? f1 : (p == 1 ? f2 : f0);
  const double fr = p == 0 ? f2 : (p == 1 ? f0 : f1);
  const double share = ((c - fp) / (fq - fp)) * ((c - fp) / (fr - fp));
  return one ? area * share : area * (1.0 - share);
}

template <int DEG>
__global__ __launch_bounds__(kBlock) void isoline_measure_kernel(
    int nc, const double* __restrict__ xy, const int* __restrict__ cell_dofs, int n,
    const double* __restrict__ f, const flow_isoline_levels L,
    double* __restrict__ partials) {
  constexpr int NS = DEG == 1 ? 1 : 4;
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = c < nc;
  CellValues<DEG> v = load_values<DEG>(nc, live ? c : 0, n, cell_dofs, f);
  const CellNodes<DEG> g = load_nodes<DEG>(xy, nc, live ? c : 0, v);
  const bool use = live && v.ok;
  // the sub-triangles with finite values: what a level below all of them adds
  double whole = 0.0;
#pragma unroll
  for (int s = 0; s < NS; ++s)
    whole += finite3(v.f[sub_node<DEG>(s, 0)], v.f[sub_node<DEG>(s, 1)],
                     v.f[sub_node<DEG>(s, 2)])
                 ? g.sub_area
                 : 0.0;
#pragma unroll 1
  for (int l = 0; l < L.n; ++l) {
    const double lev = L.c[l];
    double len = 0.0, area = 0.0;
    if (use && v.lo < lev && lev <= v.hi) {
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        const Node& A = g.n[sub_node<DEG>(s, 0)];
        const Node& B = g.n[sub_node<DEG>(s, 1)];
        const Node& C = g.n[sub_node<DEG>(s, 2)];
        if (!finite3(A.f, B.f, C.f)) continue;
        area += area_above(A.f, B.f, C.f, lev, g.sub_area);
        if (crossed(A.f, B.f, C.f, lev)) {
          Crossing p, q;
          segment(A, B, C, lev, g.cw, p, q);
          const double dx = q.x - p.x, dy = q.y - p.y;
          len += sqrt(dx * dx + dy * dy);
        }
      }
    } else if (use && lev <= v.lo) {
      area = whole;
    }
    len = block_sum_once(len);
    if (threadIdx.x == 0) partials[(size_t)(2 * l) * gridDim.x + blockIdx.x] = len;
    __syncthreads();   // block_sum_once keeps no barrier for a second call
    area = block_sum_once(area);
    if (threadIdx.x == 0) partials[(size_t)(2 * l + 1) * gridDim.x + blockIdx.x] = area;
    __syncthreads();
  }
}

// block q adds row q of the partials in a fixed order (form_sum_kernel's shape)
__global__ __launch_bounds__(kBlock) void isoline_sum_kernel(
    int nparts, const double* __restrict__ partials, double* __restrict__ out) {
  const double* row = partials + (size_t)blockIdx.x * nparts;
  double s = 0.0;
  for (int i = threadIdx.x; i < nparts; i += blockDim.x) s += row[i];
  s = block_sum_once(s);
  if (threadIdx.x == 0) out[blockIdx.x] = s;
}

int check_isoline(const flow_mesh* mesh, const flow_space* V, const double* f,
                  const flow_isoline_levels* levels) {
  FLOW_REQUIRE(mesh && mesh->nc >= 1 && mesh->nc <= INT_MAX / 6, "mesh");
  FLOW_REQUIRE(mesh->c1 == 0, "isolines on strips");
  FLOW_REQUIRE(V && (V->deg == 1 || V->deg == 2) && V->n >= 1 && V->cell_dofs, "space");
  FLOW_REQUIRE(V->r1 == 0, "isolines on strips");
  FLOW_REQUIRE(f, "field");
  FLOW_REQUIRE(levels && levels->n >= 0 && levels->n <= kMaxLev,
               "isolines: at most FLOW_ISOLINE_LEVELS_PER_LAUNCH levels per launch");
  FLOW_REQUIRE(levels->base >= 0, "isolines: index of the first level");
  return FLOW_OK;
}

flow_isoline_levels padded(const flow_isoline_levels* levels) {
  flow_isoline_levels L;
  L.n = levels->n;
  L.base = levels->base;
  for (int k = 0; k < kMaxLev; ++k) L.c[k] = k < levels->n ? levels->c[k] : 0.0;
  return L;
}

}  // namespace
}  // namespace flow

using namespace flow;

extern "C" int flow_isoline_count(const flow_mesh* mesh, const flow_space* V, const double* f,
                                  const flow_isoline_levels* levels, int* count,
                                  void* stream) {
  const int rc = check_isoline(mesh, V, f, levels);
  if (rc) return rc;
  FLOW_REQUIRE(count, "count");
  if (levels->n == 0) return FLOW_OK;
  const flow_isoline_levels L = padded(levels);
  const dim3 blocks((mesh->nc + kBlock - 1) / kBlock);
  if (V->deg == 1)
    hipLaunchKernelGGL((isoline_count_kernel<1>), blocks, dim3(kBlock), 0, as_stream(stream),
                       mesh->nc, V->cell_dofs, V->n, f, L, count);
  else
    hipLaunchKernelGGL((isoline_count_kernel<2>), blocks, dim3(kBlock), 0, as_stream(stream),
                       mesh->nc, V->cell_dofs, V->n, f, L, count);
  FLOW_CHECK_LAUNCH();
  return FLOW_OK;
}

extern "C" int flow_isoline_emit(const flow_mesh* mesh, const flow_space* V, const double* f,
                                 const flow_isoline_levels* levels, const int* count,
                                 const int* offset, int capacity, double* xy, int* level,
                                 int* cell, int* keys, double* bary, void* stream) {
  const int rc = check_isoline(mesh, V, f, levels);
  if (rc) return rc;
  FLOW_REQUIRE(mesh->xy, "mesh");
  FLOW_REQUIRE(count && offset, "counts and offsets");
  FLOW_REQUIRE(capacity >= 0, "capacity");
  if (levels->n == 0 || capacity == 0) return FLOW_OK;
  FLOW_REQUIRE(xy && level && cell && keys && bary, "outputs");
  const flow_isoline_levels L = padded(levels);
  const dim3 blocks((mesh->nc + kBlock - 1) / kBlock);
  if (V->deg == 1)
    hipLaunchKernelGGL((isoline_emit_kernel<1>), blocks, dim3(kBlock), 0, as_stream(stream),
                       mesh->nc, mesh->xy, V->cell_dofs, V->n, f, L, count, offset, capacity,
                       xy, level, cell, keys, bary);
  else
    hipLaunchKernelGGL((isoline_emit_kernel<2>), blocks, dim3(kBlock), 0, as_stream(stream),
                       mesh->nc, mesh->xy, V->cell_dofs, V->n, f, L, count, offset, capacity,
                       xy, level, cell, keys, bary);
  FLOW_CHECK_LAUNCH();
  return FLOW_OK;
}

extern "C" int flow_isoline_measure(const flow_mesh* mesh, const flow_space* V,
                                    const double* f, const flow_isoline_levels* levels,
                                    double* partials, double* out, void* stream) {
  const int rc = check_isoline(mesh, V, f, levels);
  if (rc) return rc;
  FLOW_REQUIRE(mesh->xy, "mesh");
  FLOW_REQUIRE(partials && out, "pointers");
  FLOW_REQUIRE(partials != out, "in place");
  if (levels->n == 0) return FLOW_OK;
  const flow_isoline_levels L = padded(levels);
  const int nblocks = (mesh->nc + kBlock - 1) / kBlock;
  hipStream_t st = as_stream(stream);
  if (V->deg == 1)
    hipLaunchKernelGGL((isoline_measure_kernel<1>), dim3(nblocks), dim3(kBlock), 0, st,
                       mesh->nc, mesh->xy, V->cell_dofs, V->n, f, L, partials);
  else
    hipLaunchKernelGGL((isoline_measure_kernel<2>), dim3(nblocks), dim3(kBlock), 0, st,
                       mesh->nc, mesh->xy, V->cell_dofs, V->n, f, L, partials);
  hipLaunchKernelGGL(isoline_sum_kernel, dim3(2 * L.n), dim3(kBlock), 0, st, nblocks, partials,
                     out);
  FLOW_CHECK_LAUNCH();
  return FLOW_OK;
}
