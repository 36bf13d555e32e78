// The P1 triangulation of the dofs and its cut at a level: what fem.Distance
// (distance_kernels.hip), fem.Isolines (isoline_kernels.hip) and fem.Regions
// (region_kernels.hip) share.
//
// The sub-triangulation.  On P1 the cells.  On P2 every cell is cut into its
// three corner triangles (v_s, e_(s+2), e_(s+1)), s = 0, 1, 2, and the middle
// one (e_0, e_1, e_2): local dofs [v0 v1 v2 e0 e1 e2] with e_i opposite v_i as
// in fem_device.h, every sub-triangle in the cell's cyclic order.  Node
// positions come from the cell's three vertex coordinates; a mid point is
// 0.5 (v_j + v_k), the same bits in both cells at the edge (the sum commutes).
// The two vertices of a P2 edge are no neighbours: the mid point lies between.
//
// The cut of a sub-triangle at the level c.  A node is on the set side or not
// (Isolines: f >= c; Regions: the dof is inside).  Where the three nodes are
// not all on one side,
//   * one node P is alone on its side (lone_node), Q and R follow it in
//     cyclic order (pick);
//   * the cut runs between the crossings of the sub-edges P-Q and P-R;
//   * the crossing of the sub-edge with global dofs a < b is
//     x_a + t (x_b - x_a), t = (c - f_a) / (f_b - f_a): always from the lower
//     dof to the higher and without contraction (cross), so that the two
//     cells at an edge compute the same bits.
//
// No private memory: the callers unroll over the sub-triangles, so local nodes
// are constants, and the node that is alone is turned into values by selects.
// Device code, and the host side of the entry points that launch it.
#pragma once
#include <climits>
#include <cmath>

#include "fem_device.h"

namespace flow {

// sub-triangles of a cell, and those that hold one of its nodes: P1 nodes and
// P2 vertices lie in one, P2 edge dofs in three
template <int DEG>
constexpr int kSubTris = DEG == 1 ? 1 : 4;
template <int DEG>
constexpr int kSubTrisAtNode = DEG == 1 ? 1 : 3;

// local nodes of sub-triangle s (compile-time after unrolling)
template <int DEG>
__device__ __forceinline__ constexpr int sub_node(int s, int k) {
  if (DEG == 1) return k;
  if (s == 3) return 3 + k;
  // corner s: (v_s, e_(s+2), e_(s+1))
  return k == 0 ? s : (k == 1 ? 3 + (s + 2) % 3 : 3 + (s + 1) % 3);
}

// the k-th sub-triangle of the cell that holds local node i: its two other
// local nodes (la, lb), in the triangle's cyclic order behind the node
// (tests/distance_reference.py lists the same triples).  For a P2 edge dof:
// the corner triangles at the edge's two ends, then the middle.
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

// One lane per dof over its row of the vector contribution map (vptr / vsrc,
// entry l*nc + c: local node l of cell c): fn(i, c, la, lb, da, db, in) for
// every sub-triangle that holds the node -- local node i of cell c, the two
// other local nodes and their global dofs, `in` iff both lie in [0, n) (fn
// must not use them as indices otherwise).  ok is cleared by a row or an entry
// that leaves the map and by such a dof; a row is not walked with ok cleared.
template <int DEG, class Fn>
__device__ __forceinline__ void for_each_sub_triangle_at(
    int node, int nc, int n, const int* __restrict__ cell_dofs,
    const int* __restrict__ vptr, const int* __restrict__ vsrc, bool& ok, Fn fn) {
  constexpr int NL = Elem<DEG>::NL;
  const int p0 = vptr[node], p1 = vptr[node + 1];
  ok = ok && p0 >= 0 && p1 >= p0 && p1 <= NL * nc;
#pragma unroll 1
  for (int t = ok ? p0 : 0, te = ok ? p1 : 0; t < te; ++t) {
    const int s = vsrc[t];
    if (s < 0 || s >= NL * nc) {
      ok = false;
      continue;
    }
    const int i = s / nc, c = s - i * nc;
#pragma unroll
    for (int k = 0; k < kSubTrisAtNode<DEG>; ++k) {
      if (k > 0 && i < 3) break;      // a vertex lies in one sub-triangle
      int la, lb;
      sub_triangle<DEG>(i, k, la, lb);
      const int da = cell_dofs[la * nc + c], db = cell_dofs[lb * nc + c];
      const bool in = da >= 0 && da < n && db >= 0 && db < n;
      ok = ok && in;
      fn(i, c, la, lb, da, db, in);
    }
  }
}

__device__ __forceinline__ bool finite1(double a) { return fabs(a) < __builtin_inf(); }

__device__ __forceinline__ bool finite3(double a, double b, double c) {
  return finite1(a) && finite1(b) && finite1(c);
}

struct Pt {
  double x, y, l0, l1, l2;   // position, barycentric coordinates in the parent cell
};

struct Node {
  int d;             // global dof
  double f;          // value
  Pt p;
};

template <class T>
__device__ __forceinline__ T select3(int p, T a, T b, T c) {
  return p == 0 ? a : (p == 1 ? b : c);
}

// a, b or c for p = 0, 1, 2, field by field: selects, no indexed copy
__device__ __forceinline__ Node pick(int p, const Node& a, const Node& b, const Node& c) {
  return Node{select3(p, a.d, b.d, c.d), select3(p, a.f, b.f, c.f),
              Pt{select3(p, a.p.x, b.p.x, c.p.x), select3(p, a.p.y, b.p.y, c.p.y),
                 select3(p, a.p.l0, b.p.l0, c.p.l0), select3(p, a.p.l1, b.p.l1, c.p.l1),
                 select3(p, a.p.l2, b.p.l2, c.p.l2)}};
}

__device__ __forceinline__ double edge_mid(double a, double b) { return 0.5 * (a + b); }

// the points of a cell's 3 / 6 local nodes from its vertex coordinates
template <int DEG>
__device__ __forceinline__ void load_points(const double* __restrict__ xy, int nc, int c,
                                            Pt (&p)[Elem<DEG>::NL]) {
  const double x0 = xy[0 * nc + c], x1 = xy[1 * nc + c], x2 = xy[2 * nc + c];
  const double y0 = xy[3 * nc + c], y1 = xy[4 * nc + c], y2 = xy[5 * nc + c];
  p[0] = Pt{x0, y0, 1.0, 0.0, 0.0};
  p[1] = Pt{x1, y1, 0.0, 1.0, 0.0};
  p[2] = Pt{x2, y2, 0.0, 0.0, 1.0};
  if constexpr (DEG == 2) {
    p[3] = Pt{edge_mid(x1, x2), edge_mid(y1, y2), 0.0, 0.5, 0.5};
    p[4] = Pt{edge_mid(x0, x2), edge_mid(y0, y2), 0.5, 0.0, 0.5};
    p[5] = Pt{edge_mid(x0, x1), edge_mid(y0, y1), 0.5, 0.5, 0.0};
  }
}

// one coordinate of local node m from the three vertex coordinates, for a
// caller whose m is no constant: load_points' expressions behind selects
__device__ __forceinline__ double node_coord(int m, double v0, double v1, double v2) {
  return m < 3 ? select3(m, v0, v1, v2)
               : select3(m - 3, edge_mid(v1, v2), edge_mid(v0, v2), edge_mid(v0, v1));
}

// the node alone on its side among three that are not all on one: its place p
// (the two behind it in cyclic order are pick(p, B, C, A) and pick(p, C, A, B)),
// and whether it is the set one
struct Lone {
  int p;
  bool one;
};

__device__ __forceinline__ Lone lone_node(bool s0, bool s1, bool s2) {
  const bool one = (s0 + s1 + s2) == 1;
  return Lone{one ? (s0 ? 0 : (s1 ? 1 : 2)) : (!s0 ? 0 : (!s1 ? 1 : 2)), one};
}

struct Crossing {
  int a, b;          // the sub-edge, a < b
  Pt p;
};

// the crossing of the sub-edge between u and v, from the lower dof
__device__ __forceinline__ Crossing cross(const Node& u, const Node& v, double level) {
#pragma clang fp contract(off)
  const int lo = u.d < v.d ? 0 : 1;   // the place of the lower dof in (u, v)
  const Node a = pick(lo, u, v, v), b = pick(lo, v, u, u);
  const double t = (level - a.f) / (b.f - a.f);
  return Crossing{a.d, b.d,
                  Pt{a.p.x + t * (b.p.x - a.p.x), a.p.y + t * (b.p.y - a.p.y),
                     a.p.l0 + t * (b.p.l0 - a.p.l0), a.p.l1 + t * (b.p.l1 - a.p.l1),
                     a.p.l2 + t * (b.p.l2 - a.p.l2)}};
}

// ---- the host side -----------------------------------------------------------
// strips: the entry point's "... on strips" message
inline int check_p12_mesh_space(const flow_mesh* mesh, const flow_space* V,
                                const char* strips, bool need_xy) {
  FLOW_REQUIRE(mesh && mesh->nc >= 1 && mesh->nc <= INT_MAX / 6 && (!need_xy || mesh->xy),
               "mesh");
  FLOW_REQUIRE(mesh->c1 == 0, strips);
  FLOW_REQUIRE(V && (V->deg == 1 || V->deg == 2) && V->n >= 1 && V->cell_dofs, "space");
  FLOW_REQUIRE(V->r1 == 0, strips);
  return FLOW_OK;
}

// kernel<1> or kernel<2> on blocks of kBlock lanes
#define FLOW_LAUNCH_BY_DEGREE(deg, kernel, blocks, st, ...)                          \
  do {                                                                               \
    if ((deg) == 1)                                                                  \
      hipLaunchKernelGGL((kernel<1>), blocks, dim3(kBlock), 0, st, __VA_ARGS__);     \
    else                                                                             \
      hipLaunchKernelGGL((kernel<2>), blocks, dim3(kBlock), 0, st, __VA_ARGS__);     \
  } while (0)

// nsweeps Jacobi sweeps between two buffers: sweep(src, dst, flag) enqueues one.
// A sweep that lowers nothing has reached the fixed point, whatever the sweeps
// before it did: only the last one of the batch reports.
template <class T, class Sweep>
int jacobi_sweeps(const flow_space* V, int nsweeps, T* buf_a, T* buf_b, int* flag,
                  Sweep sweep) {
  FLOW_REQUIRE(V->vptr && V->vsrc, "vector contribution map");
  FLOW_REQUIRE(nsweeps >= 1, "sweeps");
  FLOW_REQUIRE(buf_a && buf_b && flag, "pointers");
  FLOW_REQUIRE(buf_a != buf_b, "in place");
  for (int k = 0; k < nsweeps; ++k)
    sweep((k & 1) ? buf_b : buf_a, (k & 1) ? buf_a : buf_b,
          k == nsweeps - 1 ? flag : nullptr);
  FLOW_CHECK_LAUNCH();
  return FLOW_OK;
}

}  // namespace flow
