// Connected components of a level set and their measures (flow_amd/fem/
// regions.py): the kernels behind fem.Regions.
//
// The graph is the P1 triangulation of the dofs (distance_kernels.hip,
// isoline_kernels.hip): on P1 the cells; on P2 every cell cut into its three
// corner triangles (v_s, e_(s+2), e_(s+1)) and the middle one (e_0, e_1, e_2),
// local dofs [v0 v1 v2 e0 e1 e2] with e_i opposite v_i.  A dof is INSIDE iff
// its value is finite and f >= c (side 0) or f < c (side 1).  Two inside dofs
// joined by a sub-edge are in one component; a component's label is its
// smallest dof.
//
//   flow_region_init            label[i] = inside(i) ? i : -1.
//   flow_region_sweeps          Jacobi between two int buffers, one lane per
//                               dof over its row of the vector contribution
//                               map: the minimum over the dof and its inside
//                               neighbours, then one pointer jump.
//   flow_region_moments         one lane per cell: per sub-triangle slot
//                               s*nc + cell the owning component and the
//                               integrals of 1, x, y and g_a over the piece.
//   flow_region_segment_sum     one block per (component, row): the sum of
//                               the row over the component's slots.
//   flow_region_segment_minmax  the same with min and max, over dofs.
//
// No atomics; no LDS but the block reductions; no private memory: the
// sub-triangles are unrolled, so their local nodes are constants, and the node
// that is alone on its side is turned into values by selects.
//
// Index limits: rows of the map are entries l*nc + c < 6 nc, slots are
// s*nc + c < 4 nc: 6 * nc < 2^31 is asked for, as by the neighbours.
#include <climits>
#include <cmath>

#include "fem_device.h"

namespace flow {
namespace {

__device__ __forceinline__ bool finite1(double a) { return fabs(a) < __builtin_inf(); }

__device__ __forceinline__ bool is_inside(double f, double c, int side) {
  return finite1(f) && (side == 0 ? f >= c : f < c);
}

// ---- init --------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void region_init_kernel(
    int n, const double* __restrict__ f, double c, int side, int* __restrict__ label) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  label[i] = is_inside(f[i], c, side) ? i : -1;
}

// ---- sweeps ------------------------------------------------------------------
// the k-th sub-triangle of the cell that holds local node i: its two other
// local nodes (sub_triangle of distance_kernels.hip, restated).  P1 nodes and
// P2 vertices lie in one (k = 0), P2 edge dofs in three.
template <int DEG>
__device__ __forceinline__ void sub_neighbours(int i, int k, int& la, int& lb) {
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

// one lane per dof.  Invariant of the iteration: a label is the index of an
// inside dof of the same component and is <= the dof, so old[m] below is a
// legal read; a label or an index that is not (a corrupt map, a buffer that is
// no iterate) is never used as an index and the dof is written as -1.
template <int DEG>
__global__ __launch_bounds__(kBlock) void region_sweep_kernel(
    int nc, const int* __restrict__ cell_dofs, int n, const int* __restrict__ vptr,
    const int* __restrict__ vsrc, const int* __restrict__ old, int* __restrict__ out,
    int* __restrict__ flag) {
  constexpr int NL = Elem<DEG>::NL;
  constexpr int NT = DEG == 1 ? 1 : 3;
  const int node = blockIdx.x * blockDim.x + threadIdx.x;
  if (node >= n) return;
  const int mine = old[node];
  if (mine < 0) {            // outside: stays outside
    out[node] = -1;
    return;
  }
  const int p0 = vptr[node], p1 = vptr[node + 1];
  bool ok = p0 >= 0 && p1 >= p0 && p1 <= NL * nc && mine <= node;
  int best = mine;
#pragma unroll 1
  for (int t = ok ? p0 : 0, te = ok ? p1 : 0; t < te; ++t) {
    const int s = vsrc[t];
    if (s < 0 || s >= NL * nc) {
      ok = false;
      continue;
    }
    const int i = s / nc, c = s - i * nc;
#pragma unroll
    for (int k = 0; k < NT; ++k) {
      if (k > 0 && i < 3) break;      // a vertex lies in one sub-triangle
      int la, lb;
      sub_neighbours<DEG>(i, k, la, lb);
      const int da = cell_dofs[la * nc + c], db = cell_dofs[lb * nc + c];
      const bool in = da >= 0 && da < n && db >= 0 && db < n;
      ok = ok && in;
      const int ma = old[in ? da : node], mb = old[in ? db : node];
      best = ma >= 0 && ma < best ? ma : best;
      best = mb >= 0 && mb < best ? mb : best;
    }
  }
  // the pointer jump: best is in [0, mine], mine <= node < n
  const int jump = old[ok ? best : node];
  ok = ok && jump >= 0 && jump <= best;
  out[node] = ok ? jump : -1;
  // every lane that lowered its label stores the same 1: a plain vector store
  if (flag != nullptr && ok && jump < mine) *flag = 1;
}

// ---- moments -----------------------------------------------------------------
struct Pt {
  double x, y, l0, l1, l2;   // position, barycentric coordinates in the parent cell
};

struct RNode {
  int d;             // global dof
  bool in;           // inside
  int id;            // compact id of its component, < 0 outside
  double f;
  Pt p;
};

__device__ __forceinline__ RNode pick(int p, const RNode& a, const RNode& b, const RNode& c) {
  RNode r;
  r.d = p == 0 ? a.d : (p == 1 ? b.d : c.d);
  r.in = p == 0 ? a.in : (p == 1 ? b.in : c.in);
  r.id = p == 0 ? a.id : (p == 1 ? b.id : c.id);
  r.f = p == 0 ? a.f : (p == 1 ? b.f : c.f);
  r.p.x = p == 0 ? a.p.x : (p == 1 ? b.p.x : c.p.x);
  r.p.y = p == 0 ? a.p.y : (p == 1 ? b.p.y : c.p.y);
  r.p.l0 = p == 0 ? a.p.l0 : (p == 1 ? b.p.l0 : c.p.l0);
  r.p.l1 = p == 0 ? a.p.l1 : (p == 1 ? b.p.l1 : c.p.l1);
  r.p.l2 = p == 0 ? a.p.l2 : (p == 1 ? b.p.l2 : c.p.l2);
  return r;
}

// the crossing of the sub-edge between u and v: Isolines', from the lower dof
// to the higher and without contraction, so that the two cells at an edge
// compute the same bits
__device__ __forceinline__ Pt cross(const RNode& u, const RNode& v, double c) {
#pragma clang fp contract(off)
  const bool lo = u.d < v.d;
  const RNode& a = lo ? u : v;
  const RNode& b = lo ? v : u;
  const double t = (c - a.f) / (b.f - a.f);
  Pt r;
  r.x = a.p.x + t * (b.p.x - a.p.x);
  r.y = a.p.y + t * (b.p.y - a.p.y);
  r.l0 = a.p.l0 + t * (b.p.l0 - a.p.l0);
  r.l1 = a.p.l1 + t * (b.p.l1 - a.p.l1);
  r.l2 = a.p.l2 + t * (b.p.l2 - a.p.l2);
  return r;
}

__device__ __forceinline__ Pt mid(const Pt& a, const Pt& b) {
  return Pt{0.5 * (a.x + b.x), 0.5 * (a.y + b.y), 0.5 * (a.l0 + b.l0), 0.5 * (a.l1 + b.l1),
            0.5 * (a.l2 + b.l2)};
}

// local nodes of sub-triangle s (compile-time after unrolling)
template <int DEG>
__device__ __forceinline__ constexpr int sub_node(int s, int k) {
  if (DEG == 1) return k;
  if (s == 3) return 3 + k;
  // corner s: (v_s, e_(s+2), e_(s+1))
  return k == 0 ? s : (k == 1 ? 3 + (s + 2) % 3 : 3 + (s + 1) % 3);
}

// acc += the integrals of 1, x, y and g_a over the triangle (a, b, c): the
// edge-midpoint rule, exact for degree 2; the area as an absolute value
template <int GDEG, int NCOMP>
__device__ __forceinline__ void add_triangle(const Pt& a, const Pt& b, const Pt& c,
                                             const double (*U)[Elem<GDEG>::NL],
                                             double acc[3 + NCOMP]) {
  const double area =
      0.5 * fabs((b.x - a.x) * (c.y - a.y) - (c.x - a.x) * (b.y - a.y));
  const double w = area * (1.0 / 3.0);
  const Pt m0 = mid(a, b), m1 = mid(b, c), m2 = mid(c, a);
  acc[0] += area;
  acc[1] += w * (m0.x + m1.x + m2.x);
  acc[2] += w * (m0.y + m1.y + m2.y);
  if constexpr (NCOMP > 0) {
    const double L0[3] = {m0.l0, m0.l1, m0.l2};
    const double L1[3] = {m1.l0, m1.l1, m1.l2};
    const double L2[3] = {m2.l0, m2.l1, m2.l2};
#pragma unroll
    for (int q = 0; q < NCOMP; ++q)
      acc[3 + q] +=
          w * (eval_at<GDEG>(U[q], L0) + eval_at<GDEG>(U[q], L1) + eval_at<GDEG>(U[q], L2));
  }
}

// one lane per cell
template <int DEG, int GDEG, int NCOMP>
__global__ __launch_bounds__(kBlock) void region_moments_kernel(
    int nc, const double* __restrict__ xy, const int* __restrict__ cell_dofs, int n,
    const double* __restrict__ f, double lev, const int* __restrict__ ids,
    const int* __restrict__ g_dofs, int ng, const double* __restrict__ g,
    int* __restrict__ key, double* __restrict__ vals) {
  constexpr int NL = Elem<DEG>::NL;
  constexpr int GL = Elem<GDEG>::NL;
  constexpr int NS = DEG == 1 ? 1 : 4;
  constexpr int NR = 3 + NCOMP;
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nc) return;
  const size_t nslots = (size_t)NS * nc;
  const double x0 = xy[0 * nc + c], x1 = xy[1 * nc + c], x2 = xy[2 * nc + c];
  const double y0 = xy[3 * nc + c], y1 = xy[4 * nc + c], y2 = xy[5 * nc + c];
  RNode nd[NL];
  bool ok = true;
#pragma unroll
  for (int l = 0; l < NL; ++l) {
    const int d = cell_dofs[l * nc + c];
    const bool in = d >= 0 && d < n;
    ok = ok && in;
    nd[l].d = d;
    nd[l].f = f[in ? d : 0];
    nd[l].id = in ? ids[d] : -1;
    nd[l].in = nd[l].id >= 0;
  }
  nd[0].p = Pt{x0, y0, 1.0, 0.0, 0.0};
  nd[1].p = Pt{x1, y1, 0.0, 1.0, 0.0};
  nd[2].p = Pt{x2, y2, 0.0, 0.0, 1.0};
  if constexpr (NL == 6) {
    nd[3].p = Pt{0.5 * (x1 + x2), 0.5 * (y1 + y2), 0.0, 0.5, 0.5};
    nd[4].p = Pt{0.5 * (x0 + x2), 0.5 * (y0 + y2), 0.5, 0.0, 0.5};
    nd[5].p = Pt{0.5 * (x0 + x1), 0.5 * (y0 + y1), 0.5, 0.5, 0.0};
  }
  double U[NCOMP > 0 ? NCOMP : 1][GL];
  if constexpr (NCOMP > 0) {
#pragma unroll
    for (int l = 0; l < GL; ++l) {
      const int d = g_dofs[l * nc + c];
      const bool in = d >= 0 && d < ng;
      ok = ok && in;
#pragma unroll
      for (int q = 0; q < NCOMP; ++q) U[q][l] = g[(size_t)q * ng + (in ? d : 0)];
    }
  }
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const RNode& A = nd[sub_node<DEG>(s, 0)];
    const RNode& B = nd[sub_node<DEG>(s, 1)];
    const RNode& C = nd[sub_node<DEG>(s, 2)];
    const int nin = A.in + B.in + C.in;
    const bool piece = ok && nin > 0 && finite1(A.f) && finite1(B.f) && finite1(C.f);
    double acc[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) acc[r] = 0.0;
    if (piece) {
      if (nin == 3) {
        add_triangle<GDEG, NCOMP>(A.p, B.p, C.p, U, acc);
      } else {
        // the node alone on its side, and the two behind it in cyclic order
        const bool one = nin == 1;
        const int p = one ? (A.in ? 0 : (B.in ? 1 : 2)) : (!A.in ? 0 : (!B.in ? 1 : 2));
        const RNode P = pick(p, A, B, C), Q = pick(p, B, C, A), R = pick(p, C, A, B);
        const Pt pq = cross(P, Q, lev), pr = cross(P, R, lev);
        if (one) {
          add_triangle<GDEG, NCOMP>(P.p, pq, pr, U, acc);
        } else {
          // inside Q and R, outside P: the quadrilateral Q, R, pr, pq cut by
          // the diagonal Q - pr
          add_triangle<GDEG, NCOMP>(Q.p, R.p, pr, U, acc);
          add_triangle<GDEG, NCOMP>(Q.p, pr, pq, U, acc);
        }
      }
    }
    const size_t slot = (size_t)s * nc + c;
    if (key != nullptr) key[slot] = piece ? (A.in ? A.id : (B.in ? B.id : C.id)) : -1;
#pragma unroll
    for (int r = 0; r < NR; ++r) vals[(size_t)r * nslots + slot] = acc[r];
  }
}

// ---- segment reductions ------------------------------------------------------
// block (k, row): lanes stride over perm[offsets[k] .. offsets[k+1]) in a fixed
// assignment, each adding its entries in ascending order, then the fixed-order
// block sum: the same inputs give the same bits
__global__ __launch_bounds__(kBlock) void region_segment_sum_kernel(
    int count, const int* __restrict__ offsets, const int* __restrict__ perm, int nslots,
    const double* __restrict__ vals, double* __restrict__ out) {
  const int k = blockIdx.x, row = blockIdx.y;
  int lo = offsets[k], hi = offsets[k + 1];
  lo = lo < 0 ? 0 : lo;
  hi = hi > nslots ? nslots : hi;
  const double* v = vals + (size_t)row * nslots;
  double s = 0.0;
  for (int t = lo + (int)threadIdx.x; t < hi; t += kBlock) {
    const int j = perm[t];
    s += j >= 0 && j < nslots ? v[j] : 0.0;
  }
  s = block_sum_once(s);
  if (threadIdx.x == 0) out[(size_t)row * count + k] = s;
}

// min and max commute and are exact: no order to fix
__global__ __launch_bounds__(kBlock) void region_segment_minmax_kernel(
    int count, const int* __restrict__ offsets, const int* __restrict__ perm, int n,
    const double* __restrict__ vals, double* __restrict__ out_min,
    double* __restrict__ out_max) {
  __shared__ double part_lo[4], part_hi[4];
  const int k = blockIdx.x, row = blockIdx.y;
  int first = offsets[k], last = offsets[k + 1];
  first = first < 0 ? 0 : first;
  last = last > n ? n : last;
  const double* v = vals + (size_t)row * n;
  double lo = __builtin_inf(), hi = -__builtin_inf();
  for (int t = first + (int)threadIdx.x; t < last; t += kBlock) {
    const int j = perm[t];
    if (j >= 0 && j < n) {
      const double x = v[j];
      lo = x < lo ? x : lo;
      hi = x > hi ? x : hi;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double a = __shfl_down(lo, off, 64), b = __shfl_down(hi, off, 64);
    lo = a < lo ? a : lo;
    hi = b > hi ? b : hi;
  }
  if ((threadIdx.x & 63) == 0) {
    part_lo[threadIdx.x >> 6] = lo;
    part_hi[threadIdx.x >> 6] = hi;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < 4; ++w) {
      lo = part_lo[w] < lo ? part_lo[w] : lo;
      hi = part_hi[w] > hi ? part_hi[w] : hi;
    }
    out_min[(size_t)row * count + k] = lo;
    out_max[(size_t)row * count + k] = hi;
  }
}

int check_region(const flow_mesh* mesh, const flow_space* V) {
  FLOW_REQUIRE(mesh && mesh->nc >= 1 && mesh->nc <= INT_MAX / 6, "mesh");
  FLOW_REQUIRE(mesh->c1 == 0, "regions on strips");
  FLOW_REQUIRE(V && (V->deg == 1 || V->deg == 2) && V->n >= 1 && V->cell_dofs, "space");
  FLOW_REQUIRE(V->r1 == 0, "regions on strips");
  return FLOW_OK;
}

template <int DEG, int GDEG, int NCOMP>
void launch_moments(const flow_mesh* mesh, const flow_space* V, const double* f, double level,
                    const int* ids, const flow_space* G, const double* g, int* key,
                    double* vals, hipStream_t st) {
  const dim3 blocks((mesh->nc + kBlock - 1) / kBlock);
  hipLaunchKernelGGL((region_moments_kernel<DEG, GDEG, NCOMP>), blocks, dim3(kBlock), 0, st,
                     mesh->nc, mesh->xy, V->cell_dofs, V->n, f, level, ids,
                     NCOMP > 0 ? G->cell_dofs : nullptr, NCOMP > 0 ? G->n : 0, g, key, vals);
}

template <int DEG>
void launch_moments_deg(int gdeg, int ncomp, const flow_mesh* mesh, const flow_space* V,
                        const double* f, double level, const int* ids, const flow_space* G,
                        const double* g, int* key, double* vals, hipStream_t st) {
  if (ncomp == 0)
    launch_moments<DEG, 1, 0>(mesh, V, f, level, ids, G, g, key, vals, st);
  else if (gdeg == 1 && ncomp == 1)
    launch_moments<DEG, 1, 1>(mesh, V, f, level, ids, G, g, key, vals, st);
  else if (gdeg == 1)
    launch_moments<DEG, 1, 2>(mesh, V, f, level, ids, G, g, key, vals, st);
  else if (ncomp == 1)
    launch_moments<DEG, 2, 1>(mesh, V, f, level, ids, G, g, key, vals, st);
  else
    launch_moments<DEG, 2, 2>(mesh, V, f, level, ids, G, g, key, vals, st);
}

}  // namespace
}  // namespace flow

using namespace flow;

extern "C" int flow_region_init(const flow_space* V, const double* f, double level, int side,
                                int* label, void* stream) {
  FLOW_REQUIRE(V && V->n >= 1, "space");
  FLOW_REQUIRE(V->r1 == 0, "regions on strips");
  FLOW_REQUIRE(f && label, "pointers");
  FLOW_REQUIRE(std::isfinite(level), "regions: the level must be finite");
  FLOW_REQUIRE(side == 0 || side == 1, "regions: side 0 (f >= level) or 1 (f < level)");
  const dim3 blocks((V->n + kBlock - 1) / kBlock);
  hipLaunchKernelGGL(region_init_kernel, blocks, dim3(kBlock), 0, as_stream(stream), V->n, f,
                     level, side, label);
  FLOW_CHECK_LAUNCH();
  return FLOW_OK;
}

extern "C" int flow_region_sweeps(const flow_mesh* mesh, const flow_space* V, int nsweeps,
                                  int* buf_a, int* buf_b, int* flag, void* stream) {
  const int rc = check_region(mesh, V);
  if (rc) return rc;
  FLOW_REQUIRE(V->vptr && V->vsrc, "vector contribution map");
  FLOW_REQUIRE(nsweeps >= 1, "sweeps");
  FLOW_REQUIRE(buf_a && buf_b && flag, "pointers");
  FLOW_REQUIRE(buf_a != buf_b, "in place");
  hipStream_t st = as_stream(stream);
  const dim3 blocks((V->n + kBlock - 1) / kBlock);
  for (int k = 0; k < nsweeps; ++k) {
    const int* src = (k & 1) ? buf_b : buf_a;
    int* dst = (k & 1) ? buf_a : buf_b;
    // a sweep that lowers nothing has reached the fixed point, whatever the
    // sweeps before it did: only the last one of the batch reports
    int* fl = k == nsweeps - 1 ? flag : nullptr;
    if (V->deg == 1)
      hipLaunchKernelGGL((region_sweep_kernel<1>), blocks, dim3(kBlock), 0, st, mesh->nc,
                         V->cell_dofs, V->n, V->vptr, V->vsrc, src, dst, fl);
    else
      hipLaunchKernelGGL((region_sweep_kernel<2>), blocks, dim3(kBlock), 0, st, mesh->nc,
                         V->cell_dofs, V->n, V->vptr, V->vsrc, src, dst, fl);
  }
  FLOW_CHECK_LAUNCH();
  return FLOW_OK;
}

extern "C" int flow_region_moments(const flow_mesh* mesh, const flow_space* V, const double* f,
                                   double level, const int* ids, const flow_space* G,
                                   int ncomp, const double* g, int* key, double* vals,
                                   void* stream) {
  const int rc = check_region(mesh, V);
  if (rc) return rc;
  FLOW_REQUIRE(mesh->xy, "mesh");
  FLOW_REQUIRE(f && ids && vals, "pointers");
  FLOW_REQUIRE(std::isfinite(level), "regions: the level must be finite");
  FLOW_REQUIRE(ncomp >= 0 && ncomp <= 2, "regions: 0, 1 or 2 components of g");
  if (ncomp > 0) {
    FLOW_REQUIRE(G && (G->deg == 1 || G->deg == 2) && G->n >= 1 && G->cell_dofs,
                 "space of g");
    FLOW_REQUIRE(G->r1 == 0, "regions on strips");
    FLOW_REQUIRE(g, "g");
  }
  hipStream_t st = as_stream(stream);
  const int gdeg = ncomp > 0 ? G->deg : 1;
  if (V->deg == 1)
    launch_moments_deg<1>(gdeg, ncomp, mesh, V, f, level, ids, G, g, key, vals, st);
  else
    launch_moments_deg<2>(gdeg, ncomp, mesh, V, f, level, ids, G, g, key, vals, st);
  FLOW_CHECK_LAUNCH();
  return FLOW_OK;
}

extern "C" int flow_region_segment_sum(int count, const int* offsets, const int* perm,
                                       int nrows, int nslots, const double* vals, double* out,
                                       void* stream) {
  FLOW_REQUIRE(count >= 0 && nrows >= 0 && nslots >= 0, "sizes");
  FLOW_REQUIRE(nrows <= 65535, "regions: at most 65535 rows");
  if (count == 0 || nrows == 0) return FLOW_OK;
  FLOW_REQUIRE(offsets && perm && vals && out, "pointers");
  FLOW_REQUIRE(vals != out, "in place");
  hipLaunchKernelGGL(region_segment_sum_kernel, dim3(count, nrows), dim3(kBlock), 0,
                     as_stream(stream), count, offsets, perm, nslots, vals, out);
  FLOW_CHECK_LAUNCH();
  return FLOW_OK;
}

extern "C" int flow_region_segment_minmax(int count, const int* offsets, const int* perm,
                                          int nrows, int n, const double* vals,
                                          double* out_min, double* out_max, void* stream) {
  FLOW_REQUIRE(count >= 0 && nrows >= 0 && n >= 0, "sizes");
  FLOW_REQUIRE(nrows <= 65535, "regions: at most 65535 rows");
  if (count == 0 || nrows == 0) return FLOW_OK;
  FLOW_REQUIRE(offsets && perm && vals && out_min && out_max, "pointers");
  FLOW_REQUIRE(vals != out_min && vals != out_max && out_min != out_max, "in place");
  hipLaunchKernelGGL(region_segment_minmax_kernel, dim3(count, nrows), dim3(kBlock), 0,
                     as_stream(stream), count, offsets, perm, n, vals, out_min, out_max);
  FLOW_CHECK_LAUNCH();
  return FLOW_OK;
}
