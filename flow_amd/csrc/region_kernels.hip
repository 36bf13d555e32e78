// Connected components of a level set and their measures (flow_amd/fem/
// regions.py): the kernels behind fem.Regions.
//
// The graph is the P1 triangulation of the dofs (subtri.h).  A dof is INSIDE
// iff its value is finite and f >= c (side 0) or f < c (side 1).  Two inside
// dofs joined by a sub-edge are in one component; a component's label is its
// smallest dof.  A sub-triangle with inside and outside dofs is cut at c by
// subtri.h's rule: its crossings are Isolines'.
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
// No atomics; no LDS but the block reductions; no private memory (subtri.h).
//
// Index limits: rows of the map are entries l*nc + c < 6 nc, slots are
// s*nc + c < 4 nc: 6 * nc < 2^31 is asked for, as by the neighbours.
#include "subtri.h"

namespace flow {
namespace {

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
// one lane per dof.  Invariant of the iteration: a label is the index of an
// inside dof of the same component and is <= the dof, so old[m] below is a
// legal read; a label or an index that is not (a corrupt map, a buffer that is
// no iterate) is never used as an index and the dof is written as -1.
template <int DEG>
__global__ __launch_bounds__(kBlock) void region_sweep_kernel(
    int nc, const int* __restrict__ cell_dofs, int n, const int* __restrict__ vptr,
    const int* __restrict__ vsrc, const int* __restrict__ old, int* __restrict__ out,
    int* __restrict__ flag) {
  const int node = blockIdx.x * blockDim.x + threadIdx.x;
  if (node >= n) return;
  const int mine = old[node];
  if (mine < 0) {            // outside: stays outside
    out[node] = -1;
    return;
  }
  bool ok = mine <= node;
  int best = mine;
  for_each_sub_triangle_at<DEG>(node, nc, n, cell_dofs, vptr, vsrc, ok,
                                [&](int, int, int, int, int da, int db, bool in) {
                                  const int ma = old[in ? da : node], mb = old[in ? db : node];
                                  best = ma >= 0 && ma < best ? ma : best;
                                  best = mb >= 0 && mb < best ? mb : best;
                                });
  // the pointer jump: best is in [0, mine], mine <= node < n
  const int jump = old[ok ? best : node];
  ok = ok && jump >= 0 && jump <= best;
  out[node] = ok ? jump : -1;
  // every lane that lowered its label stores the same 1: a plain vector store
  if (flag != nullptr && ok && jump < mine) *flag = 1;
}

// ---- moments -----------------------------------------------------------------
// a node of the cell; inside iff id >= 0
struct RNode : Node {
  int id;            // compact id of its component, < 0 outside
};

__device__ __forceinline__ Pt mid(const Pt& a, const Pt& b) {
  return Pt{0.5 * (a.x + b.x), 0.5 * (a.y + b.y), 0.5 * (a.l0 + b.l0), 0.5 * (a.l1 + b.l1),
            0.5 * (a.l2 + b.l2)};
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
  constexpr int NR = 3 + NCOMP;
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nc) return;
  const size_t nslots = (size_t)kSubTris<DEG> * nc;
  Pt pts[NL];
  load_points<DEG>(xy, nc, c, pts);
  RNode nd[NL];
  bool ok = true;
#pragma unroll
  for (int l = 0; l < NL; ++l) {
    const int d = cell_dofs[l * nc + c];
    const bool in = d >= 0 && d < n;
    ok = ok && in;
    nd[l].d = d;
    nd[l].f = f[in ? d : 0];
    nd[l].p = pts[l];
    nd[l].id = in ? ids[d] : -1;
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
  for (int s = 0; s < kSubTris<DEG>; ++s) {
    const RNode& A = nd[sub_node<DEG>(s, 0)];
    const RNode& B = nd[sub_node<DEG>(s, 1)];
    const RNode& C = nd[sub_node<DEG>(s, 2)];
    const bool ain = A.id >= 0, bin = B.id >= 0, cin = C.id >= 0;
    const int nin = ain + bin + cin;
    const bool piece = ok && nin > 0 && finite3(A.f, B.f, C.f);
    double acc[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) acc[r] = 0.0;
    if (piece) {
      if (nin == 3) {
        add_triangle<GDEG, NCOMP>(A.p, B.p, C.p, U, acc);
      } else {
        // the node alone on its side, and the two behind it in cyclic order
        const Lone alone = lone_node(ain, bin, cin);
        const Node P = pick(alone.p, A, B, C), Q = pick(alone.p, B, C, A),
                   R = pick(alone.p, C, A, B);
        const Pt pq = cross(P, Q, lev).p, pr = cross(P, R, lev).p;
        if (alone.one) {
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
    if (key != nullptr) key[slot] = piece ? (ain ? A.id : (bin ? B.id : C.id)) : -1;
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
  const int rc = check_p12_mesh_space(mesh, V, "regions on strips", false);
  if (rc) return rc;
  hipStream_t st = as_stream(stream);
  const dim3 blocks((V->n + kBlock - 1) / kBlock);
  return jacobi_sweeps(V, nsweeps, buf_a, buf_b, flag, [&](const int* src, int* dst, int* fl) {
    FLOW_LAUNCH_BY_DEGREE(V->deg, region_sweep_kernel, blocks, st, mesh->nc, V->cell_dofs, V->n,
                          V->vptr, V->vsrc, src, dst, fl);
  });
}

extern "C" int flow_region_moments(const flow_mesh* mesh, const flow_space* V, const double* f,
                                   double level, const int* ids, const flow_space* G,
                                   int ncomp, const double* g, int* key, double* vals,
                                   void* stream) {
  const int rc = check_p12_mesh_space(mesh, V, "regions on strips", true);
  if (rc) return rc;
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
