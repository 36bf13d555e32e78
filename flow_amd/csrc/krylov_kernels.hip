// The device-resident Krylov drivers of a single GPU (K12) -- Chronopoulos-Gear
// CG, BiCGStab, GMRES(m) -- with the two-level and V-cycle preconditioners,
// on the products, reductions and read-backs of la_kernels.hip.  How the
// solvers stop (the sticky flag S[kDone], decided on the device) is described
// there; the host side of it is run_batches() and gmres_cycle() below.
#include "common.h"
#include "csr_stream.h"
#include "la_internal.h"

namespace flow {

// The two kernels of a multigrid level (flow_mg) on the same tiles:
//   UP = 0:  y = c - A x                     (A = Ah, x = c = r:  t = r - Ah r)
//   UP = 1:  y = A x + w dinv (c + t)        (A = Ps, x = x_{l+1}, c = r)
//            DOTS: the workgroup's shares of c.y and y.y -> gpart / rpart
template <int UP, bool DOTS>
__global__ __launch_bounds__(kBlock) void mg_level_kernel(
    const int* __restrict__ rowptr, const int* __restrict__ cols,
    const double* __restrict__ vals, const int* __restrict__ rowblocks,
    const double* __restrict__ x, const double* __restrict__ c,
    const double* __restrict__ t, const double* __restrict__ dinv, double omega,
    double* __restrict__ y, double* __restrict__ gpart,
    double* __restrict__ rpart, const double* __restrict__ stop) {
  __shared__ double prod[kTile];
  if (stopped(stop)) return;
  int r, r1;
  const double s =
      stream_tile_row_sum(rowptr, cols, vals, rowblocks, x, prod, r, r1);
  double g = 0.0, rr = 0.0;
  if (r < r1) {
    const double ci = c[r];
    if (UP) {
      const double yi = s + omega * dinv[r] * (ci + t[r]);
      y[r] = yi;
      if (DOTS) {
        g = ci * yi;
        rr = yi * yi;
      }
    } else {
      y[r] = ci - s;
    }
  }
  if (DOTS) {
    g = block_sum(g);
    rr = block_sum(rr);
    if (threadIdx.x == 0) {
      gpart[blockIdx.x] = g;
      rpart[blockIdx.x] = rr;
    }
  }
}

// The up-sweep of a multigrid level in ONE launch (flow_mg's two-launch form):
//   y = Ps x' + w dinv (2 c - Ah c)
// -- both products of the workgroup's rows, over row blocks that hold at most a
// tile of nonzeros of Ps AND of Ah; DOTS as in mg_level_kernel.  y must not be c.
template <bool DOTS>
__global__ __launch_bounds__(kBlock) void mg_up2_kernel(
    const int* __restrict__ rowblocks, const int* __restrict__ p_rowptr,
    const int* __restrict__ p_cols, const double* __restrict__ p_vals,
    const int* __restrict__ a_rowptr, const int* __restrict__ a_cols,
    const double* __restrict__ a_vals, const double* __restrict__ xc,
    const double* __restrict__ c, const double* __restrict__ dinv, double omega,
    double* __restrict__ y, double* __restrict__ gpart,
    double* __restrict__ rpart, const double* __restrict__ stop,
    int own_lo, int own_hi) {
  __shared__ double prod_p[kTile];
  __shared__ double prod_a[kTile];
  if (stopped(stop)) return;
  const int tile = xcd_tile(blockIdx.x, gridDim.x);
  const int r0 = rowblocks[tile];
  const int r1 = rowblocks[tile + 1];
  const int r = r0 + threadIdx.x;
  double ci = 0.0, di = 0.0;       // (early: with the tiles' own loads)
  if (r < r1) {
    ci = c[r];
    di = dinv[r];
  }
  const double sp = stream_rows_sum(r0, r1, p_rowptr, p_cols, p_vals, xc, prod_p);
  const double sa = stream_rows_sum(r0, r1, a_rowptr, a_cols, a_vals, c, prod_a);
  double g = 0.0, rr = 0.0;
  if (r < r1) {
    const double yi = sp + omega * di * (2.0 * ci - sa);
    y[r] = yi;
    // (K15: a rank that also forms y on its first ghost layer counts its OWN
    // rows only; the ghost rows are counted by their owners)
    if (DOTS && r >= own_lo && r < own_hi) {
      g = ci * yi;
      rr = yi * yi;
    }
  }
  if (DOTS) {
    g = block_sum(g);
    rr = block_sum(rr);
    if (threadIdx.x == 0) {
      gpart[blockIdx.x] = g;
      rpart[blockIdx.x] = rr;
    }
  }
}

// Chronopoulos-Gear CG scalars from (gamma_new, delta, z.z) partials
// gamma = r.z and z.z: nparts partials each in gpart / rpart;
// delta = z.w: ndelta partials in dpart (left there by the SpMV itself)
// (kScalarBlock = 1024: la_internal.h)
__global__ __launch_bounds__(kScalarBlock) void cg_scalar_kernel(
    int nparts, int ndelta, int first, const double* __restrict__ gpart,
    const double* __restrict__ rpart, const double* __restrict__ dpart,
    double rtol2, double atol2, double* __restrict__ S) {
  __shared__ double wsum[3][kScalarBlock / 64];
  if (stopped(S + kDone)) return;
  double g = 0.0, rr = 0.0;
  for (int i = threadIdx.x; i < nparts; i += kScalarBlock) {
    g += load_scalar(gpart + i);
    rr += load_scalar(rpart + i);
  }
  // four independent chains keep the loads of the long list in flight
  double d0 = 0.0, d1 = 0.0, d2 = 0.0, d3 = 0.0;
  int i = threadIdx.x;
  for (; i + 3 * kScalarBlock < ndelta; i += 4 * kScalarBlock) {
    d0 += load_scalar(dpart + i);
    d1 += load_scalar(dpart + i + kScalarBlock);
    d2 += load_scalar(dpart + i + 2 * kScalarBlock);
    d3 += load_scalar(dpart + i + 3 * kScalarBlock);
  }
  for (; i < ndelta; i += kScalarBlock) d0 += load_scalar(dpart + i);
  double d = (d0 + d1) + (d2 + d3);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    g += __shfl_down(g, off, 64);
    d += __shfl_down(d, off, 64);
    rr += __shfl_down(rr, off, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    wsum[0][threadIdx.x >> 6] = g;
    wsum[1][threadIdx.x >> 6] = d;
    wsum[2][threadIdx.x >> 6] = rr;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    g = d = rr = 0.0;
    for (int w = 0; w < kScalarBlock / 64; ++w) {
      g += wsum[0][w];
      d += wsum[1][w];
      rr += wsum[2][w];
    }
  }
  if (threadIdx.x == 0) {
    double alpha, beta;
    if (first) {
      beta = 0.0;
      alpha = (d != 0.0) ? g / d : 0.0;
      // the stopping test of the whole solve, in the PRECONDITIONED norm like
      // PETSc's KSPCG (its default, which the reference's `solve` runs with):
      // |B r| <= max(rtol |B b|, atol), z = B r, S[kB2] = |B b|^2
      const double b2 = load_scalar(S + kB2);
      store_scalar(S + kTarget2, fmax(rtol2 * b2, atol2));
      store_scalar(S + kIter, 0.0);
      // a guarded start (first == 2: flow_cg_solve_guarded) that leaves a
      // LARGER preconditioned residual than the zero start would, |B r0| >
      // |B b|, is rejected: S[kDone] = 5 turns everything behind this kernel
      // into no-ops -- x still holds the start --, the host swaps in the
      // fallback.  (What a far start costs these recurrences is attainable
      // accuracy: the recurrence residual drifts from the true one in
      // proportion to the largest residual seen, and from zero -- the
      // reference's start -- that is |b|.)
      if (first == 2 && rr > b2) {
        store_scalar(S + kConvIt, 0.0);
        store_scalar(S + kRes2, rr);
        store_scalar(S + kDone, 5.0);
        return;
      }
    } else {
      const double g_old = load_scalar(S + kGamma);
      const double a_old = load_scalar(S + kAlpha);
      beta = (g_old != 0.0) ? g / g_old : 0.0;
      const double den = (a_old != 0.0) ? d - beta * g / a_old : 0.0;
      alpha = (den != 0.0) ? g / den : 0.0;
    }
    // rr = z.z belongs to the iterate x_k, k = S[kIter] updates behind the
    // start: the first one that passes the test (or is not a number) stops
    // the iteration for good
    const double k = load_scalar(S + kIter);
    const bool nan = !(rr == rr);
    if (nan || rr <= load_scalar(S + kTarget2)) {
      store_scalar(S + kConvIt, k);
      store_scalar(S + kDone, nan ? 2.0 : 1.0);
      alpha = beta = 0.0;
    }
    store_scalar(S + kIter, k + 1.0);
    store_scalar(S + kGamma, g);
    store_scalar(S + kAlpha, alpha);
    store_scalar(S + kBeta, beta);
    store_scalar(S + kRes2, rr);
  }
}

// p = z + beta p ; s = w + beta s ; x += alpha p ; r -= alpha s ; z = dinv r
// (want_z = 0: z is produced afterwards by the two-level preconditioner)
// DOTS (needs want_z, gridDim.x <= kRedBlocks): the block's shares of r.z and
// z.z go to partial[blockIdx.x] / partial[2*kRedBlocks + blockIdx.x].
// own != nullptr (sharded solves: the vectors cover ghost rows too): the dots
// only count the entries with own[i] = 1
template <bool DOTS>
__global__ __launch_bounds__(kBlock) void cg_update_kernel(
    int n, const double* __restrict__ S, const double* __restrict__ dinv,
    const double* __restrict__ w, double* __restrict__ z, double* __restrict__ p,
    double* __restrict__ s, double* __restrict__ x, double* __restrict__ r,
    int want_z, double* __restrict__ partial,
    const double* __restrict__ own) {
  if (stopped(S + kDone)) return;
  const double alpha = load_scalar(S + kAlpha);
  const double beta = load_scalar(S + kBeta);
  double g = 0.0, rr = 0.0;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += gridDim.x * blockDim.x) {
    const double pi = z[i] + beta * p[i];
    const double si = w[i] + beta * s[i];
    p[i] = pi;
    s[i] = si;
    x[i] += alpha * pi;
    const double ri = r[i] - alpha * si;
    r[i] = ri;
    if (want_z) {
      const double zi = dinv ? dinv[i] * ri : ri;
      z[i] = zi;
      if (DOTS && (!own || own[i] != 0.0)) {   // (select, not multiply:
        g += ri * zi;                            // ghost entries may be NaN)
        rr += zi * zi;
      }
    }
  }
  if (DOTS) {
    g = block_sum(g);
    rr = block_sum(rr);
    if (threadIdx.x == 0) {
      partial[blockIdx.x] = g;
      partial[2 * kRedBlocks + blockIdx.x] = rr;
    }
  }
}

// (the three templates above are launched from shard_kernels.hip too: compiled
// here, once)
FLOW_KRYLOV_INSTANCES(template)

// ---------------------------------------------------------------------------
// two-level additive preconditioner  z = D^-1 r + P Ac^-1 P^T r
// (Jacobi + piecewise-constant aggregate coarse space, dense coarse inverse)
// ---------------------------------------------------------------------------
// rc[a] = sum of r over the dofs of aggregate a that lie in [r0, r1): one
// wavefront per aggregate, fixed order => reproducible
__global__ __launch_bounds__(kBlock) void coarse_restrict_kernel(
    int nc, const int* __restrict__ agg_ptr, const int* __restrict__ agg_dofs,
    const double* __restrict__ r, int r0, int r1, double* __restrict__ rc,
    const double* __restrict__ stop) {
  if (stopped(stop)) return;
  const int lane = threadIdx.x & 63;
  for (int a = blockIdx.x * 4 + (threadIdx.x >> 6); a < nc; a += gridDim.x * 4) {
    double sum = 0.0;
    for (int k = agg_ptr[a] + lane; k < agg_ptr[a + 1]; k += 64) {
      const int d = agg_dofs[k];
      if (d >= r0 && d < r1) sum += r[d];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off, 64);
    if (lane == 0) rc[a] = sum;
  }
}

// zc = Ainv rc (dense fp32 rows of lda floats, fp64 accumulation): one
// wavefront per row, float4 loads; rc 16-byte aligned, nc entries.  (rc and zc
// are per-lane -- vector -- loads: the stale reads common.h describes were
// only ever observed on wave-uniform loads, which go through the scalar cache.)
__global__ __launch_bounds__(kBlock) void coarse_gemv_kernel(
    int nc, int lda, const float* __restrict__ Ainv,
    const double* __restrict__ rc, double* __restrict__ zc,
    const double* __restrict__ stop) {
  if (stopped(stop)) return;
  const int lane = threadIdx.x & 63;
  const int nq = lda >> 2;
  for (int row = blockIdx.x * 4 + (threadIdx.x >> 6); row < nc;
       row += gridDim.x * 4) {
    const float4* __restrict__ a =
        reinterpret_cast<const float4*>(Ainv + static_cast<size_t>(row) * lda);
    const double2* __restrict__ x = reinterpret_cast<const double2*>(rc);
    double s0 = 0.0, s1 = 0.0;
    for (int q = lane; q < nq; q += 64) {
      const float4 v = a[q];
      double2 x0, x1;
      if (4 * q + 3 < nc) {
        x0 = x[2 * q];
        x1 = x[2 * q + 1];
      } else {   // last quad of a row whose length is not a multiple of 4
        const int j = 4 * q;
        x0.x = rc[j];
        x0.y = (j + 1 < nc) ? rc[j + 1] : 0.0;
        x1.x = (j + 2 < nc) ? rc[j + 2] : 0.0;
        x1.y = 0.0;
      }
      s0 += static_cast<double>(v.x) * x0.x + static_cast<double>(v.z) * x1.x;
      s1 += static_cast<double>(v.y) * x0.y + static_cast<double>(v.w) * x1.y;
    }
    double sum = s0 + s1;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off, 64);
    if (lane == 0) zc[row] = sum;
  }
}

// z = dinv r + zc[agg_of]  on dofs [0, n) of pre-offset arrays
// DOTS (gridDim.x <= kRedBlocks): also the block's shares of r.z and z.z, as
// in cg_update_kernel
template <bool DOTS>
__global__ __launch_bounds__(kBlock) void coarse_prolong_kernel(
    int n, const int* __restrict__ agg_of, const double* __restrict__ dinv,
    const double* __restrict__ r, const double* __restrict__ zc,
    double* __restrict__ z, double* __restrict__ partial,
    const double* __restrict__ stop) {
  if (stopped(stop)) return;
  double g = 0.0, rr = 0.0;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += gridDim.x * blockDim.x) {
    const int a = agg_of[i];
    const double ri = r[i];
    const double zi = dinv[i] * ri + (a >= 0 ? zc[a] : 0.0);
    z[i] = zi;
    if (DOTS) {
      g += ri * zi;
      rr += zi * zi;
    }
  }
  if (DOTS) {
    g = block_sum(g);
    rr = block_sum(rr);
    if (threadIdx.x == 0) {
      partial[blockIdx.x] = g;
      partial[2 * kRedBlocks + blockIdx.x] = rr;
    }
  }
}

static int check_coarse(const flow_coarse* C, int n) {
  FLOW_REQUIRE(C->nc > 0 && C->n == n, "coarse space size");
  FLOW_REQUIRE(C->agg_ptr && C->agg_dofs && C->agg_of && C->Ainv,
               "coarse space pointers");
  FLOW_REQUIRE(C->lda >= C->nc && C->lda % 4 == 0 &&
                   reinterpret_cast<uintptr_t>(C->Ainv) % 16 == 0,
               "coarse inverse: row stride must be a multiple of 4 floats, "
               "base 16-byte aligned");
  return FLOW_OK;
}

// z = M^-1 r with the two-level preconditioner; rc, zc: lda doubles each.
// partial != nullptr: the prolongation also leaves the shares of r.z and z.z
// of its *nparts workgroups there.
static int two_level(const flow_coarse* C, const double* dinv, const double* r,
                     double* z, double* rc, double* zc, hipStream_t st,
                     double* partial = nullptr, int* nparts = nullptr,
                     const double* stop = nullptr) {
  const int g = grid_for(C->nc, 4, kMaxGrid);
  hipLaunchKernelGGL(coarse_restrict_kernel, dim3(g), dim3(kBlock), 0, st, C->nc,
                     C->agg_ptr, C->agg_dofs, r, 0, C->n, rc, stop);
  hipLaunchKernelGGL(coarse_gemv_kernel, dim3(g), dim3(kBlock), 0, st, C->nc,
                     C->lda, C->Ainv, rc, zc, stop);
  if (partial) {
    const int gp = grid_for(C->n, kBlock, kRedBlocks);
    hipLaunchKernelGGL(coarse_prolong_kernel<true>, dim3(gp), dim3(kBlock), 0,
                       st, C->n, C->agg_of, dinv, r, zc, z, partial, stop);
    *nparts = gp;
  } else {
    hipLaunchKernelGGL(coarse_prolong_kernel<false>, dim3(grid_for(C->n)),
                       dim3(kBlock), 0, st, C->n, C->agg_of, dinv, r, zc, z,
                       partial, stop);
  }
  FLOW_CHECK_LAUNCH();
  return FLOW_OK;
}

// ---------------------------------------------------------------------------
// smoothed-aggregation multigrid V(1,1) cycle (flow_mg, include/flow_hip.h)
// ---------------------------------------------------------------------------
// multigrid V-cycle (flow_mg)
int check_mg(const flow_mg* M, int n) {
  FLOW_REQUIRE(M->nlevels >= 1 && M->nlevels <= FLOW_MG_MAX_LEVELS, "mg levels");
  FLOW_REQUIRE(M->omega > 0.0 && M->omega < 2.0, "mg damping");
  int rows = n;
  for (int l = 0; l + 1 < M->nlevels; ++l) {
    int rc = check_operator(&M->Ah[l]);
    if (rc) return rc;
    if ((rc = check_operator(&M->Ps[l]))) return rc;
    if ((rc = check_operator(&M->R[l]))) return rc;
    FLOW_REQUIRE(M->Ah[l].kind == 0 && M->Ps[l].kind == 0 && M->R[l].kind == 0,
                 "mg operators are scalar");
    FLOW_REQUIRE(M->Ah[l].n == rows && M->Ps[l].n == rows, "mg level sizes");
    FLOW_REQUIRE(M->dinv[l] && M->t[l], "mg level vectors");
    FLOW_REQUIRE(l == 0 || (M->r[l] && M->x[l]), "mg level vectors");
    if (M->C[0].rowptr) {     // the two-launch form: every level carries it
      if ((rc = check_operator(&M->C[l]))) return rc;
      FLOW_REQUIRE(M->C[l].kind == 0 && M->C[l].n == M->R[l].n &&
                       M->up_rowblocks[l] && M->up_nblocks[l] > 0,
                   "mg two-launch form: C and the common row blocks");
    }
    rows = M->R[l].n;
  }
  const int last = M->nlevels - 1;
  FLOW_REQUIRE(M->nc == rows && M->Ainv && M->lda >= M->nc && M->lda % 4 == 0 &&
                   reinterpret_cast<uintptr_t>(M->Ainv) % 16 == 0,
               "mg coarsest level");
  FLOW_REQUIRE(last == 0 || (M->r[last] && M->x[last] &&
                             reinterpret_cast<uintptr_t>(M->r[last]) % 16 == 0),
               "mg coarsest vectors");
  return FLOW_OK;
}

// z = V-cycle(r) from level l0 down (l0 = 0: the whole hierarchy; the sharded
// pressure solve runs the levels >= 1 replicated: l0 = 1, r0 = the summed
// coarse residual).  gpart != nullptr (l0 = 0 only): the last kernel also
// leaves the *nparts (= Ps[0].nblocks) workgroup shares of r.z in gpart and z.z
// in rpart
int vcycle(const flow_mg* M, const double* r0, double* z0, hipStream_t st,
           double* gpart, double* rpart, int* nparts, const double* stop,
           int l0) {
  const int L = M->nlevels;
  int rc;
  double* const none = nullptr;
  const bool fused = M->C[0].rowptr != nullptr;
  for (int l = l0; l + 1 < L; ++l) {
    const double* r = l == l0 ? r0 : M->r[l];
    if (fused) {
      // r_{l+1} = C r,  C = R (I - Ah)
      if ((rc = apply(&M->C[l], r, M->r[l + 1], st, nullptr, stop))) return rc;
      continue;
    }
    const flow_operator* A = &M->Ah[l];
    // t = r - Ah r ; r_{l+1} = R t
    hipLaunchKernelGGL((mg_level_kernel<0, false>), dim3(A->nblocks), dim3(kBlock),
                       0, st, A->rowptr, A->cols, A->vals[0], A->rowblocks, r, r,
                       none, none, M->omega, M->t[l], none, none, stop);
    if ((rc = apply(&M->R[l], M->t[l], M->r[l + 1], st, nullptr, stop)))
      return rc;
  }
  {
    const double* r = l0 == L - 1 ? r0 : M->r[L - 1];
    double* x = l0 == L - 1 ? z0 : M->x[L - 1];
    hipLaunchKernelGGL(coarse_gemv_kernel, dim3(grid_for(M->nc, 4, kMaxGrid)),
                       dim3(kBlock), 0, st, M->nc, M->lda, M->Ainv, r, x, stop);
  }
  for (int l = L - 2; l >= l0; --l) {
    const double* r = l == l0 ? r0 : M->r[l];
    double* x = l == l0 ? z0 : M->x[l];
    const flow_operator* P = &M->Ps[l];
    const bool with_dots = l == 0 && gpart;
    if (fused) {
      // x = Ps x_{l+1} + w D^-1 (2 r - Ah r)
      const flow_operator* A = &M->Ah[l];
      const dim3 grid(M->up_nblocks[l]);
      if (with_dots)
        hipLaunchKernelGGL(mg_up2_kernel<true>, grid, dim3(kBlock), 0, st,
                           M->up_rowblocks[l], P->rowptr, P->cols, P->vals[0],
                           A->rowptr, A->cols, A->vals[0], M->x[l + 1], r,
                           M->dinv[l], M->omega, x, gpart, rpart, stop);
      else
        hipLaunchKernelGGL(mg_up2_kernel<false>, grid, dim3(kBlock), 0, st,
                           M->up_rowblocks[l], P->rowptr, P->cols, P->vals[0],
                           A->rowptr, A->cols, A->vals[0], M->x[l + 1], r,
                           M->dinv[l], M->omega, x, none, none, stop);
      if (with_dots) *nparts = M->up_nblocks[l];
      continue;
    }
    // x = Ps x_{l+1} + w D^-1 (r + t)
    if (with_dots) {
      hipLaunchKernelGGL((mg_level_kernel<1, true>), dim3(P->nblocks),
                         dim3(kBlock), 0, st, P->rowptr, P->cols, P->vals[0],
                         P->rowblocks, M->x[l + 1], r, M->t[l], M->dinv[l],
                         M->omega, x, gpart, rpart, stop);
      *nparts = P->nblocks;
    } else {
      hipLaunchKernelGGL((mg_level_kernel<1, false>), dim3(P->nblocks),
                         dim3(kBlock), 0, st, P->rowptr, P->cols, P->vals[0],
                         P->rowblocks, M->x[l + 1], r, M->t[l], M->dinv[l],
                         M->omega, x, none, none, stop);
    }
  }
  FLOW_CHECK_LAUNCH();
  return FLOW_OK;
}

// Work of cg(): [reductions | r z w p s | z.w partials of the SpMV | rc zc |
// r.z, z.z partials of the V-cycle's last kernel]
// partials the V-cycle's last kernel leaves (r.z and z.z each)
static inline int mg_parts(const flow_mg* M) {
  if (!M || M->nlevels < 2) return 0;
  return M->C[0].rowptr ? M->up_nblocks[0] : M->Ps[0].nblocks;
}

static inline size_t cg_work_len(const flow_operator* A, const flow_coarse* C,
                                 const flow_mg* M) {
  const size_t N = op_size(A);
  return FLOW_REDUCE_WORK + 5 * N + dot_parts(A) + 2 +
         (C ? 2 * static_cast<size_t>(C->lda) : 0) +
         2 * static_cast<size_t>(mg_parts(M));
}

// The host side of the stopping test of CG and BiCGStab.  Iterations are
// enqueued in batches -- iteration(k) enqueues number k --; the device decides
// which iterate passes the test (the solver's scalar kernel) and turns
// everything behind it into no-ops, so a batch may overshoot: the first one is
// `first_check` iterations (the caller's guess of what the solve needs), later
// ones `check_every`; the state S is read back behind every batch.
// FLOW_OK: converged -- or, with rejected != nullptr (a guarded start),
// *rejected = true: the start was dropped and x still holds it.  `solver` and
// `norm` ("|B r|", "|r|") only enter the messages.
static int run_batches(const char* solver, const char* norm, int maxit,
                       int first_check, int check_every, const double* S,
                       hipStream_t st, bool* rejected,
                       const std::function<int(int)>& iteration,
                       int* iters_host, double* resid_host) {
  if (rejected) *rejected = false;
  double state[kNumSlots];
  int launched = 0, rc;
  while (true) {
    const int batch = (launched == 0 && first_check > 0) ? first_check
                                                         : check_every;
    const int todo = (maxit - launched < batch) ? maxit - launched : batch;
    for (int k = 0; k < todo; ++k)
      if ((rc = iteration(launched + k))) return rc;
    FLOW_CHECK_LAUNCH();
    launched += todo;
    if ((rc = read_state(S, state, st))) return rc;
    const double res2 = state[kRes2];
    if (state[kDone] == 2.0 || !(res2 == res2)) {
      *iters_host = static_cast<int>(state[kConvIt]);
      *resid_host = res2;
      set_error("%s broke down (NaN residual) at iteration %d", solver,
                *iters_host);
      return FLOW_NOT_CONVERGED;
    }
    if (state[kDone] == 1.0) {
      *iters_host = static_cast<int>(state[kConvIt]);
      *resid_host = sqrt(res2);
      return FLOW_OK;
    }
    if (state[kDone] == 5.0 && rejected) {
      *rejected = true;
      *iters_host = 0;
      *resid_host = sqrt(res2);
      return FLOW_OK;
    }
    if (launched >= maxit) {
      *iters_host = launched;
      *resid_host = sqrt(res2);
      set_error("%s did not converge in %d iterations: %s = %.3e > %.3e", solver,
                launched, norm, sqrt(res2), sqrt(state[kTarget2]));
      return FLOW_NOT_CONVERGED;
    }
  }
}

// Chronopoulos-Gear CG.  Per iteration: update (x, r, p, s) -> preconditioner
// -> SpMV -> scalars; the three dot products ride in those kernels (r.z and z.z
// in whichever kernel produces z, z.w in the SpMV), so no vector is re-read for
// a reduction.
static int cg(const flow_operator* A, const double* dinv,
              const flow_coarse* C, const flow_mg* M, const double* b,
              double* x, double rtol, double atol, int maxit, int check_every,
              int first_check, double* work, int* iters_host,
              double* resid_host, hipStream_t st, bool* rejected = nullptr) {
  // rejected != nullptr: the start vector is guarded (cg_scalar_kernel); when
  // it is rejected, *rejected = true, x is the start still, FLOW_OK
  const int N = op_size(A);
  const int nd = dot_parts(A);
  double* partial = work;
  double* S = work + 3 * kRedBlocks;
  double* r = work + FLOW_REDUCE_WORK;
  double* z = r + N;
  double* w = z + N;
  double* p = w + N;
  double* s = p + N;
  double* dpart = s + N;
  // coarse vectors (two-level only), 16-byte aligned
  double* crc = dpart + nd + ((N + nd) & 1);
  double* czc = crc + (C ? C->lda : 0);
  double* mpart = czc + (C ? C->lda : 0);     // V-cycle partials (multigrid only)
  const int nm = mg_parts(M);
  const double* gpart = M ? mpart : partial;
  const double* rpart = M ? mpart + nm : partial + 2 * kRedBlocks;
  const int gv = grid_for(N);
  const int gu = grid_for(N, kBlock, kRedBlocks);   // update with fused dots
  int np = 0, rc;

  const double* stop = S + kDone;
  double* const r_ = r;     // (for the lambdas below, whose `r` is a status)
  const double rtol2 = rtol * rtol, atol2 = atol * atol;
  if ((rc = fill(kNumSlots, 0.0, S, st))) return rc;
  if ((rc = fill(2 * N, 0.0, p, st))) return rc;      // p, s
  // |B b|^2, B the preconditioner (z is free until the start below)
  if (C) {
    if ((rc = two_level(C, dinv, b, z, crc, czc, st))) return rc;
  } else if (M) {
    if ((rc = vcycle(M, b, z, st))) return rc;
  } else if (dinv) {
    hipLaunchKernelGGL(vmul_kernel, dim3(gv), dim3(kBlock), 0, st, N, 1.0, dinv,
                       b, z);
  }
  const double* Bb = (C || M || dinv) ? z : b;
  if ((rc = dots(N, 1, Bb, Bb, Bb, Bb, Bb, Bb, partial, &np, st))) return rc;
  hipLaunchKernelGGL(finish_kernel, dim3(1), dim3(kBlock), 0, st, np, 1, 0,
                     partial, S + kB2);
  // r = b - A x ; z = B r ; w = A z
  if ((rc = apply(A, x, w, st))) return rc;
  hipLaunchKernelGGL(residual_kernel, dim3(gv), dim3(kBlock), 0, st, N, b, w,
                     dinv, r, z);
  if (C && (rc = two_level(C, dinv, r, z, crc, czc, st))) return rc;
  if (M && (rc = vcycle(M, r, z, st))) return rc;
  if ((rc = apply(A, z, w, st, dpart))) return rc;
  if ((rc = dots(N, 3, r, z, z, w, z, z, partial, &np, st))) return rc;
  hipLaunchKernelGGL(cg_scalar_kernel, dim3(1), dim3(kScalarBlock), 0, st, np,
                     nd, rejected ? 2 : 1, partial, partial + 2 * kRedBlocks,
                     dpart, rtol2, atol2, S);
  FLOW_CHECK_LAUNCH();

  // one iteration: the same launches with the same arguments every time (the
  // tolerances only enter the FIRST scalar kernel above)
  auto body = [&]() -> int {
    int r;
    if (C) {
      hipLaunchKernelGGL(cg_update_kernel<false>, dim3(gv), dim3(kBlock), 0,
                         st, N, S, dinv, w, z, p, s, x, r_, 0, partial,
                         static_cast<const double*>(nullptr));
      if ((r = two_level(C, dinv, r_, z, crc, czc, st, partial, &np, stop)))
        return r;
    } else if (M) {
      hipLaunchKernelGGL(cg_update_kernel<false>, dim3(gv), dim3(kBlock), 0,
                         st, N, S, dinv, w, z, p, s, x, r_, 0, partial,
                         static_cast<const double*>(nullptr));
      if ((r = vcycle(M, r_, z, st, mpart, mpart + nm, &np, stop))) return r;
    } else {
      hipLaunchKernelGGL(cg_update_kernel<true>, dim3(gu), dim3(kBlock), 0, st,
                         N, S, dinv, w, z, p, s, x, r_, 1, partial,
                         static_cast<const double*>(nullptr));
      np = gu;
    }
    if ((r = apply(A, z, w, st, dpart, stop))) return r;
    hipLaunchKernelGGL(cg_scalar_kernel, dim3(1), dim3(kScalarBlock), 0, st,
                       np, nd, 0, gpart, rpart, dpart, 0.0, 0.0, S);
    FLOW_CHECK_LAUNCH();
    return FLOW_OK;
  };
  // ... replayed as a HIP graph where the launch rate bounds the iteration
  // (graph_replay.hip; never while the SpMV is being timed with events)
  hipGraphExec_t graph = nullptr;
  int graph_nodes = 0;
  if (replay_wanted(N, kReplayCg) && g_spmv_profile.ev == nullptr) {
    KeyHash key;
    key.pod(0x6367ull);       // "cg"
    key_operator(key, A);
    key.obj(C).obj(M).pod(dinv).pod(x).pod(work).pod(N);
    if ((rc = replay_prepare(key.h, kReplayCg, st, body, &graph, &graph_nodes))) return rc;
  }

  // (the start is only read back with the first batch)
  return run_batches(
      "CG", "|B r|", maxit, first_check, check_every, S, st, rejected,
      [&](int) { return graph ? replay_launch(graph, graph_nodes, st) : body(); },
      iters_host, resid_host);
}

// ---------------------------------------------------------------------------
// BiCGStab (right-preconditioned with Jacobi), van der Vorst 1992
// ---------------------------------------------------------------------------
// mode 0: rho_new = partial0 ; beta = (rho_new/rho)(alpha/omega)
// mode 1: alpha = rho_new / partial0 (= rhat.v)
// mode 2: omega = partial0/partial1 (= t.s / t.t); rho = rho_new;
//         rho_new = partial2 (= rhat.r of the NEW r needs another pass: see 3)
// mode 3: rho_new = partial0 (rhat.r), res2 = partial1 (r.r)
// mode 3 also decides convergence on the device (see `stopped`): first != 0
// sets the target from |b|^2; the first r that passes the test freezes x, r, p.
__global__ __launch_bounds__(kBlock) void bicg_scalar_kernel(
    int nparts, int mode, int first, double rtol2, double atol2,
    const double* __restrict__ partial, double* __restrict__ S) {
  if (stopped(S + kDone)) return;
  double a = 0.0, b = 0.0;
  for (int i = threadIdx.x; i < nparts; i += kBlock) {
    a += load_scalar(partial + i);
    b += load_scalar(partial + kRedBlocks + i);
  }
  a = block_sum(a);
  b = block_sum(b);
  if (threadIdx.x != 0) return;
  if (mode == 1) {
    store_scalar(S + kAlpha, (a != 0.0) ? load_scalar(S + kRhoNew) / a : 0.0);
    if (a == 0.0) store_scalar(S + kBreak, 1.0);
  } else if (mode == 2) {
    store_scalar(S + kOmega, (b != 0.0) ? a / b : 0.0);
  } else {   // mode 3 (also used for initialisation)
    const double rho_old = load_scalar(S + kRhoNew);
    const double omega = load_scalar(S + kOmega);
    const double alpha = load_scalar(S + kAlpha);
    store_scalar(S + kRho, rho_old);
    store_scalar(S + kRhoNew, a);
    store_scalar(S + kRes2, b);
    store_scalar(S + kBeta, (rho_old != 0.0 && omega != 0.0)
                                ? (a / rho_old) * (alpha / omega)
                                : 0.0);
    if (first) {
      store_scalar(S + kTarget2, fmax(rtol2 * load_scalar(S + kB2), atol2));
      store_scalar(S + kIter, 0.0);
    }
    const double k = load_scalar(S + kIter);
    const bool nan = !(b == b);
    if (nan || b <= load_scalar(S + kTarget2)) {
      store_scalar(S + kConvIt, k);
      store_scalar(S + kDone, nan ? 2.0 : 1.0);
    }
    store_scalar(S + kIter, k + 1.0);
  }
}

// p = r + beta (p - omega v) ; y = dinv p
__global__ void bicg_p_kernel(int n, const double* __restrict__ S,
                              const double* __restrict__ dinv,
                              const double* __restrict__ r,
                              const double* __restrict__ v,
                              double* __restrict__ p, double* __restrict__ y) {
  if (stopped(S + kDone)) return;
  const double beta = load_scalar(S + kBeta);
  const double omega = load_scalar(S + kOmega);
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += gridDim.x * blockDim.x) {
    const double pi = r[i] + beta * (p[i] - omega * v[i]);
    p[i] = pi;
    y[i] = dinv ? dinv[i] * pi : pi;
  }
}

// s = r - alpha v (in place in r) ; z = dinv s
__global__ void bicg_s_kernel(int n, const double* __restrict__ S,
                              const double* __restrict__ dinv,
                              const double* __restrict__ v,
                              double* __restrict__ r, double* __restrict__ z) {
  if (stopped(S + kDone)) return;
  const double alpha = load_scalar(S + kAlpha);
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += gridDim.x * blockDim.x) {
    const double si = r[i] - alpha * v[i];
    r[i] = si;
    z[i] = dinv ? dinv[i] * si : si;
  }
}

// x += alpha y + omega z ; r = s - omega t
__global__ void bicg_x_kernel(int n, const double* __restrict__ S,
                              const double* __restrict__ y,
                              const double* __restrict__ z,
                              const double* __restrict__ t,
                              double* __restrict__ x, double* __restrict__ r) {
  if (stopped(S + kDone)) return;
  const double alpha = load_scalar(S + kAlpha);
  const double omega = load_scalar(S + kOmega);
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += gridDim.x * blockDim.x) {
    x[i] += alpha * y[i] + omega * z[i];
    r[i] -= omega * t[i];
  }
}

static int bicgstab(const flow_operator* A, const double* dinv,
                    const flow_ilu* ilu, const double* b,
                    double* x, double rtol, double atol, int maxit,
                    int check_every, int first_check, double* work,
                    int* iters_host, double* resid_host, hipStream_t st) {
  const int N = op_size(A);
  double* partial = work;
  double* S = work + 3 * kRedBlocks;
  double* r = work + FLOW_REDUCE_WORK;
  double* rhat = r + N;
  double* p = rhat + N;
  double* v = p + N;
  double* y = v + N;
  double* z = y + N;
  double* t = z + N;
  double* iwork = t + N;                  // ILU sweep buffer (ilu only)
  if (ilu) dinv = nullptr;                // y = ILU(p), z = ILU(s) below
  const int gv = grid_for(N);
  int np = 0, rc;

  if ((rc = fill(kNumSlots, 0.0, S, st))) return rc;
  if ((rc = fill(2 * N, 0.0, p, st))) return rc;      // p, v
  if ((rc = dots(N, 1, b, b, b, b, b, b, partial, &np, st))) return rc;
  hipLaunchKernelGGL(finish_kernel, dim3(1), dim3(kBlock), 0, st, np, 1, 0,
                     partial, S + kB2);
  if ((rc = apply(A, x, t, st))) return rc;
  hipLaunchKernelGGL(residual_kernel, dim3(gv), dim3(kBlock), 0, st, N, b, t,
                     static_cast<const double*>(nullptr), r,
                     static_cast<double*>(nullptr));
  hipLaunchKernelGGL(axpby_kernel, dim3(gv), dim3(kBlock), 0, st, N, 1.0, r, 0.0,
                     rhat);                           // rhat = r0
  // rho_new = rhat.r, res2 = r.r ; beta = 0 because rho_old = omega = 0
  const double rtol2 = rtol * rtol, atol2 = atol * atol;
  if ((rc = dots(N, 2, rhat, r, r, r, r, r, partial, &np, st))) return rc;
  hipLaunchKernelGGL(bicg_scalar_kernel, dim3(1), dim3(kBlock), 0, st, np, 3, 1,
                     rtol2, atol2, partial, S);
  FLOW_CHECK_LAUNCH();

  // one iteration; the device freezes x, r, p at the first residual that
  // passes the stopping test (bicg_scalar_kernel mode 3), see cg()
  auto body = [&](int) -> int {
    int rc;
    hipLaunchKernelGGL(bicg_p_kernel, dim3(gv), dim3(kBlock), 0, st, N, S, dinv,
                       r, v, p, y);
    if (ilu && (rc = ilu_apply(ilu, p, y, iwork, st))) return rc;
    if ((rc = apply(A, y, v, st))) return rc;
    if ((rc = dots(N, 1, rhat, v, v, v, v, v, partial, &np, st))) return rc;
    hipLaunchKernelGGL(bicg_scalar_kernel, dim3(1), dim3(kBlock), 0, st, np, 1,
                       0, rtol2, atol2, partial, S);
    hipLaunchKernelGGL(bicg_s_kernel, dim3(gv), dim3(kBlock), 0, st, N, S, dinv,
                       v, r, z);
    if (ilu && (rc = ilu_apply(ilu, r, z, iwork, st))) return rc;
    if ((rc = apply(A, z, t, st))) return rc;
    if ((rc = dots(N, 2, t, r, t, t, t, t, partial, &np, st))) return rc;
    hipLaunchKernelGGL(bicg_scalar_kernel, dim3(1), dim3(kBlock), 0, st, np, 2,
                       0, rtol2, atol2, partial, S);
    hipLaunchKernelGGL(bicg_x_kernel, dim3(gv), dim3(kBlock), 0, st, N, S, y, z,
                       t, x, r);
    if ((rc = dots(N, 2, rhat, r, r, r, r, r, partial, &np, st))) return rc;
    hipLaunchKernelGGL(bicg_scalar_kernel, dim3(1), dim3(kBlock), 0, st, np, 3,
                       0, rtol2, atol2, partial, S);
    return FLOW_OK;
  };
  return run_batches("BiCGStab", "|r|", maxit, first_check, check_every, S, st,
                     nullptr, body, iters_host, resid_host);
}

}  // namespace flow

using namespace flow;

// ---------------------------------------------------------------------------
// GMRES(m), right-preconditioned (Saad & Schultz 1986), classical Gram-Schmidt
// with ONE reduction per Arnoldi step:
//   w = A M^-1 V_j ; the dots w.V_k (k <= j), w.w and |V_j|^2 are summed
//   together; h_{j+1,j} follows from Pythagoras, the new basis vector is
//   formed (and scaled with that estimate) in one fused pass that also leaves
//   the partial sums of its true norm -- summed with the next step's dots and
//   put into H then.
// The Hessenberg matrix, the least-squares problem and the stopping test live
// ON THE DEVICE (gmres_step_kernel, one workgroup): the kernel that sums the
// dots also extends H, solves min |beta e1 - H y|, writes the coefficients of
// the next basis vector and of the solution update into device memory, and
// sets the solver's sticky done flag -- the Arnoldi steps are enqueued without
// the host in between (round 1 read every step's dots back: ~25 us of idle GPU
// per step), as many as the caller expects the solve to need; everything
// enqueued behind the accepted iterate returns at once.  (The sharded variant
// further down keeps this algebra on the host: its sums come out of a
// collective it has to wait for anyway.)
// Basis vectors are handled eight at a time (compile-time unrolled).
// ---------------------------------------------------------------------------
// (kGmresMax: la_internal.h)
static_assert((kGmresMax + 2) * kRedBlocks == FLOW_GMRES_PARTIALS, "gmres work");
static_assert(kGmresMax + 2 <= kMailbox, "mailbox size");
struct Coef8 {
  double c[8];
};

// block partials of w.V_k, k < NV (V_k = V + k stride) [and of w.w]
template <int NV>
__global__ __launch_bounds__(kBlock) void gmres_dots_kernel(
    int n, const double* __restrict__ w, const double* __restrict__ V,
    size_t stride, int with_ww, double* __restrict__ partial,
    double* __restrict__ ww_partial, const double* __restrict__ stop) {
  if (stopped(stop)) return;
  double acc[NV];
#pragma unroll
  for (int k = 0; k < NV; ++k) acc[k] = 0.0;
  double ww = 0.0;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += gridDim.x * blockDim.x) {
    const double wi = w[i];
#pragma unroll
    for (int k = 0; k < NV; ++k) acc[k] += wi * V[k * stride + i];
    ww += wi * wi;
  }
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const double a = block_sum(acc[k]);
    if (threadIdx.x == 0) partial[k * kRedBlocks + blockIdx.x] = a;
  }
  if (with_ww) {
    ww = block_sum(ww);
    if (threadIdx.x == 0) ww_partial[blockIdx.x] = ww;
  }
}
// (launched from shard_kernels.hip too: compiled here, once)
#define FLOW_GMRES_DOTS_DEFINE(NV)                                     \
  template __global__ void gmres_dots_kernel<NV>(                      \
      int, const double*, const double*, size_t, int, double*, double*, \
      const double*);
FLOW_GMRES_DOTS_INSTANCES(FLOW_GMRES_DOTS_DEFINE)
#undef FLOW_GMRES_DOTS_DEFINE

// out = (first ? cw w : out) + sum_{k<NV} c_k V_k ; nn_partial != nullptr: the
// block partials of |out|^2.  out may be w.
template <int NV>
__global__ __launch_bounds__(kBlock) void gmres_combine_kernel(
    int n, Coef8 coef, double cw, int first, const double* w,
    const double* __restrict__ V, size_t stride, double* out,
    double* __restrict__ nn_partial) {
  double nn = 0.0;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += gridDim.x * blockDim.x) {
    double acc = first ? (w ? cw * w[i] : 0.0) : out[i];
#pragma unroll
    for (int k = 0; k < NV; ++k) acc += coef.c[k] * V[k * stride + i];
    out[i] = acc;
    nn += acc * acc;
  }
  if (nn_partial) {
    nn = block_sum(nn);
    if (threadIdx.x == 0) nn_partial[blockIdx.x] = nn;
  }
}

// gmres_combine_kernel with the coefficients in device memory: coef[k] (k < NV)
// and, for the w term, *cw
template <int NV>
__global__ __launch_bounds__(kBlock) void gmres_combine_dev_kernel(
    int n, const double* __restrict__ coef, const double* __restrict__ cw,
    int first, const double* w, const double* __restrict__ V, size_t stride,
    double* out, double* __restrict__ nn_partial,
    const double* __restrict__ stop) {
  if (stopped(stop)) return;
  double c[NV];
#pragma unroll
  for (int k = 0; k < NV; ++k) c[k] = load_scalar(coef + k);
  const double c_w = (first && w) ? load_scalar(cw) : 0.0;
  double nn = 0.0;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += gridDim.x * blockDim.x) {
    double acc = first ? (w ? c_w * w[i] : 0.0) : out[i];
#pragma unroll
    for (int k = 0; k < NV; ++k) acc += c[k] * V[k * stride + i];
    out[i] = acc;
    nn += acc * acc;
  }
  if (nn_partial) {
    nn = block_sum(nn);
    if (threadIdx.x == 0) nn_partial[blockIdx.x] = nn;
  }
}

// (the device-resident state of one GMRES cycle, G + kGH ...: la_internal.h)

// Arnoldi step j of a cycle, the part round 1 did on the host: sums of the
// partials of w.V_k (k <= j), w.w and |V_j|^2 -> column j of H, the
// least-squares problem, the stopping test.  One workgroup; the wavefronts sum
// the value lists, thread 0 does the (tiny, serial) algebra -- O(j) per step:
// H is kept in its rotated (triangular) form R; a step re-rotates column j-1
// (its sub-diagonal has just been corrected with the true norm of V_j) and
// column j with the rotations kept from before; the triangular solve for y
// only runs behind the step that ends the cycle (`last`) or the solve.
//   S[kConvIt] = columns of this cycle that are final, S[kRes2] = the residual
//   estimate, S[kDone] = 1 converged / 2 not a number / 3 the cycle has to end
//   without a verdict (see below)
__global__ __launch_bounds__(kBlock) void gmres_step_kernel(
    int nparts, int j, int last, double beta, double target,
    const double* __restrict__ partial, double* __restrict__ G,
    double* __restrict__ S) {
  // nparts = 0: `partial` holds the nd + 1 [+ 1] values themselves, one after
  // the other (the sharded solver: summed over the ranks by the collective)
  constexpr int ld = kGmresMax + 1;
  __shared__ double val[kGmresMax + 2];
  // columns < j: rows <= col-1 rotated (R), column j-1 as H left it
  __shared__ double Hs[kGmresMax * ld];
  __shared__ double nrm[kGmresMax + 1], eta[kGmresMax];
  __shared__ double g[kGmresMax + 1], cs[kGmresMax], sn[kGmresMax], y[kGmresMax];
  if (stopped(S + kDone)) return;
  // beta < 0: the cycle's |r0| and the target are on the device (left by
  // gmres_begin_kernel: the single-GPU solver reads nothing back before the
  // cycle's steps are enqueued)
  if (beta < 0.0) {
    beta = load_scalar(S + kBeta);
    target = load_scalar(S + kTarget2);
  }
  const int nd = j + 1;
  const int nval = nd + 1 + (j > 0 ? 1 : 0);
  const int lane = threadIdx.x & 63;
  // the value lists, a wavefront each (per-lane loads, four in flight)
  // (everything an earlier launch wrote at these same addresses is read with
  // load_scalar, common.h; the loads of a lane are independent: all in flight)
  if (nparts == 0 && threadIdx.x < nval)
    val[threadIdx.x] = load_scalar(partial + threadIdx.x);
  for (int v = threadIdx.x >> 6; nparts > 0 && v < nval; v += kBlock / 64) {
    const int list = v < nd ? v : kGmresMax + (v - nd);
    const double* __restrict__ p = partial + list * kRedBlocks;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    int i = lane;
    for (; i + 192 < nparts; i += 256) {
      const double a0 = load_scalar(p + i), a1 = load_scalar(p + i + 64);
      const double a2 = load_scalar(p + i + 128), a3 = load_scalar(p + i + 192);
      s0 += a0;
      s1 += a1;
      s2 += a2;
      s3 += a3;
    }
    for (; i < nparts; i += 64) s0 += load_scalar(p + i);
    double s = (s0 + s1) + (s2 + s3);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    if (lane == 0) val[v] = s;
  }
  // the state earlier steps of the cycle left (per-lane loads as well)
  for (int i = threadIdx.x; i < j * ld; i += kBlock)
    Hs[i] = load_scalar(G + kGH + i);
  if (threadIdx.x < j) {
    nrm[threadIdx.x] = load_scalar(G + kGNrm + threadIdx.x);
    eta[threadIdx.x] = load_scalar(G + kGEta + threadIdx.x);
    cs[threadIdx.x] = load_scalar(G + kGRot + 2 * threadIdx.x);
    sn[threadIdx.x] = load_scalar(G + kGRot + 2 * threadIdx.x + 1);
    g[threadIdx.x] = load_scalar(G + kGRhs + threadIdx.x);
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  // G holds, for every finished column c: rows 0..c-1 of R (rotated) and, in
  // rows c and c+1, the UNROTATED pair (h_cc after the earlier rotations, the
  // sub-diagonal) -- the rotation c is formed from them when column c+1 comes
  // (then the sub-diagonal is final) or at the end of this step
  if (j == 0) {
    nrm[0] = beta;
    g[0] = beta;
  }
  if (j > 0) {
    // the true norm of V_j (it was scaled with the Pythagoras estimate eta)
    nrm[j] = sqrt(val[nd + 1]);
    const int c = j - 1;
    Hs[c * ld + j] = eta[c] * nrm[j];
    // rotation c, now final
    const double a = Hs[c * ld + c], bsub = Hs[c * ld + c + 1];
    const double d = hypot(a, bsub);
    cs[c] = d > 0.0 ? a / d : 1.0;
    sn[c] = d > 0.0 ? bsub / d : 0.0;
    Hs[c * ld + c] = d;
    G[kGH + c * ld + c] = d;
    G[kGRot + 2 * c] = cs[c];
    G[kGRot + 2 * c + 1] = sn[c];
    const double gc = g[c];           // (unrotated so far)
    g[c + 1] = -sn[c] * gc;
    g[c] = cs[c] * gc;
    G[kGRhs + c] = g[c];
  }
  const double nj = nrm[j];
  G[kGNrm + j] = nj;
  const double ww = val[nd] / (nj * nj);
  double sum = 0.0;
  double* col = Hs + j * ld;
  for (int k = 0; k <= j; ++k) {
    const double h = val[k] / (nj * nrm[k]);
    y[k] = h;                         // (H[j][k], for the coefficients below)
    col[k] = h;
    sum += h * h;
  }
  if (!(ww == ww) || !(nj > 0.0)) {
    store_scalar(S + kConvIt, static_cast<double>(j));
    store_scalar(S + kDone, 2.0);
    return;
  }
  const double e2 = ww - sum;
  // h_{j+1,j}^2 = |w|^2 - sum h^2 (Pythagoras: one pass over the basis instead
  // of two) cancels when w lies in the span of the basis to more than ~6
  // digits -- an invariant subspace, or simply a preconditioner that is nearly
  // exact (tiny time steps: A M^-1 ~ I, the first w is parallel to V_0 to 8
  // digits).  What is left of e2 is then rounding noise and so is the residual
  // estimate built on it: the cycle ends here, WITHOUT a verdict -- the host
  // applies the update, computes the true residual and either stops there or
  // starts the next cycle from it.  (Round 1 took e2 <= 0 for convergence: a
  // solve could return after one iteration with a true residual of 6e-9 |b|.)
  const bool lucky = !(e2 > 1.0e-12 * ww);
  const double et = e2 > 0.0 ? sqrt(e2) : 0.0;
  G[kGEta + j] = et;
  // the coefficients of V_{j+1} = (w / nrm_j - sum_k H[j][k] V_k / nrm_k) / eta_j
  // (unused when the step ends the cycle)
  if (!lucky) {
    const double inv = 1.0 / et;
    for (int k = 0; k <= j; ++k)
      store_scalar(G + kGCoef + k, -y[k] * inv / nrm[k]);
    store_scalar(G + kGCw, inv / nj);
  }
  // column j through the rotations 0 .. j-1
  for (int i = 0; i < j; ++i) {
    const double t = cs[i] * col[i] + sn[i] * col[i + 1];
    col[i + 1] = -sn[i] * col[i] + cs[i] * col[i + 1];
    col[i] = t;
  }
  col[j + 1] = et;
  for (int r = 0; r <= j + 1; ++r) G[kGH + j * ld + r] = col[r];
  G[kGRhs + j] = g[j];                // (before its own rotation)
  // residual estimate with the Pythagoras sub-diagonal: |g_{j+1}| after
  // rotation j
  const double dj = hypot(col[j], et);
  const double csj = dj > 0.0 ? col[j] / dj : 1.0;
  const double snj = dj > 0.0 ? et / dj : 0.0;
  const double resid = fabs(snj * g[j]);
  store_scalar(S + kRes2, resid);
  store_scalar(S + kConvIt, static_cast<double>(j + 1));
  const bool done = resid <= target && !lucky;
  if (done || lucky || last) {
    // y from the triangular system R y = g over the j+1 columns
    const int nc = j + 1;
    col[j] = dj;
    g[j] = csj * g[j];
    for (int i = nc - 1; i >= 0; --i) {
      double t = g[i];
      for (int c = i + 1; c < nc; ++c) t -= Hs[c * ld + i] * y[c];
      const double rii = Hs[i * ld + i];
      y[i] = rii != 0.0 ? t / rii : 0.0;
    }
    // (read by the update kernel with load_scalar: wave-uniform there)
    for (int k = 0; k < nc; ++k) store_scalar(G + kGYc + k, y[k] / nrm[k]);
    if (done) store_scalar(S + kDone, 1.0);
    if (lucky) store_scalar(S + kDone, 3.0);     // end of cycle, no verdict
  }
}

// Start of a GMRES cycle, one workgroup: |r0|^2 (list 0 of `partial`) and, the
// first time, |b|^2 (list 1; have_b2 = 0: b IS r0) -> S[kBeta] = |r0|,
// S[kTarget2] = the target max(rtol |b|, atol) (NOT squared here), and the
// verdict on the start itself: S[kDone] = 4 when r0 already passes (accept10:
// within a factor 10 -- the verification behind a cycle that stopped on the
// least-squares estimate), 2 when it is not a number.  With it the host
// enqueues the cycle's Arnoldi steps without having read anything back.
__global__ __launch_bounds__(kBlock) void gmres_begin_kernel(
    int nparts, int have_b2, int first, int accept10, double rtol, double atol,
    const double* __restrict__ partial, double* __restrict__ S) {
  double r = 0.0, b = 0.0;
  for (int i = threadIdx.x; i < nparts; i += kBlock) {
    r += load_scalar(partial + i);
    if (have_b2) b += load_scalar(partial + kRedBlocks + i);
  }
  r = block_sum(r);
  b = block_sum(b);
  if (threadIdx.x != 0) return;
  double target;
  if (first) {
    const double b2 = have_b2 ? b : r;
    target = fmax(rtol * sqrt(b2), atol);
    store_scalar(S + kB2, b2);
    store_scalar(S + kTarget2, target);
    // a start vector that leaves a LARGER residual than zero would is dropped:
    // S[kTmp] = 1 tells gmres_drop_start_kernel to put V_0 = b, x = 0
    if (have_b2 && r > b2) {
      store_scalar(S + kTmp, 1.0);
      r = b2;
    }
  } else {
    target = load_scalar(S + kTarget2);
  }
  const double beta = sqrt(r);
  store_scalar(S + kBeta, beta);
  store_scalar(S + kRes2, beta);
  store_scalar(S + kConvIt, 0.0);
  if (!(r == r))
    store_scalar(S + kDone, 2.0);
  else if (beta <= target || (accept10 && beta <= 10.0 * target))
    store_scalar(S + kDone, 4.0);
}

// behind gmres_begin_kernel of a solve that was handed a start vector: when that
// vector was worse than zero (S[kTmp] set), V_0 = b and x = 0
__global__ void gmres_drop_start_kernel(int n, const double* __restrict__ S,
                                        const double* __restrict__ b,
                                        double* __restrict__ v0,
                                        double* __restrict__ x) {
  if (load_scalar(S + kTmp) == 0.0) return;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += gridDim.x * blockDim.x) {
    v0[i] = b[i];
    x[i] = 0.0;
  }
}

// (FLOW_NV_SWITCH: la_internal.h)

// out = [accumulate ? out : cw w] + sum_{k<nv} c[k] V_k (w == nullptr: no w
// term); nn_partial as above
static int gmres_combine(int N, int nv, const double* c, double cw,
                         const double* w, const double* V, double* out,
                         double* nn_partial, bool accumulate, hipStream_t st) {
  const int g = grid_for(N, kBlock, kRedBlocks);
  if (nv == 0) {   // only the w term (cannot happen in the Arnoldi loop)
    FLOW_REQUIRE(w != nullptr, "gmres combine");
    Coef8 none = {};
    hipLaunchKernelGGL(gmres_combine_kernel<1>, dim3(g), dim3(kBlock), 0, st, N,
                       none, cw, 1, w, V, static_cast<size_t>(N), out,
                       nn_partial);
  }
  for (int k0 = 0; k0 < nv; k0 += 8) {
    const int chunk = nv - k0 < 8 ? nv - k0 : 8;
    Coef8 coef = {};
    for (int k = 0; k < chunk; ++k) coef.c[k] = c[k0 + k];
    double* nnp = (k0 + 8 >= nv) ? nn_partial : nullptr;
#define FLOW_CALL(NV)                                                          \
  hipLaunchKernelGGL(gmres_combine_kernel<NV>, dim3(g), dim3(kBlock), 0, st, N, \
                     coef, cw, (k0 == 0 && !accumulate) ? 1 : 0, w,            \
                     V + static_cast<size_t>(k0) * N, static_cast<size_t>(N),  \
                     out, nnp)
    FLOW_NV_SWITCH(chunk, FLOW_CALL)
#undef FLOW_CALL
  }
  FLOW_CHECK_LAUNCH();
  return FLOW_OK;
}

// the same with the coefficients in device memory (coef[0, nv), *cw)
int flow::gmres_combine_dev(int N, int nv, const double* coef, const double* cw,
                            const double* w, const double* V, double* out,
                            double* nn_partial, bool accumulate,
                            const double* stop, hipStream_t st) {
  const int g = grid_for(N, kBlock, kRedBlocks);
  for (int k0 = 0; k0 < nv; k0 += 8) {
    const int chunk = nv - k0 < 8 ? nv - k0 : 8;
    double* nnp = (k0 + 8 >= nv) ? nn_partial : nullptr;
#define FLOW_CALL(NV)                                                           \
  hipLaunchKernelGGL(gmres_combine_dev_kernel<NV>, dim3(g), dim3(kBlock), 0, st, \
                     N, coef + k0, cw, (k0 == 0 && !accumulate) ? 1 : 0, w,     \
                     V + static_cast<size_t>(k0) * N, static_cast<size_t>(N),   \
                     out, nnp, stop)
    FLOW_NV_SWITCH(chunk, FLOW_CALL)
#undef FLOW_CALL
  }
  FLOW_CHECK_LAUNCH();
  return FLOW_OK;
}

// The dot products of Arnoldi step j: block partials of w.V_k, k <= j, in the
// lists P + k kRedBlocks and of w.w in Pww (gd workgroups), eight basis vectors
// per launch.
static void arnoldi_dots(int N, int j, const double* w, const double* V, int gd,
                         double* P, double* Pww, const double* stop,
                         hipStream_t st) {
  for (int k0 = 0; k0 <= j; k0 += 8) {
    const int chunk = j + 1 - k0 < 8 ? j + 1 - k0 : 8;
#define FLOW_CALL(NV)                                                         \
  hipLaunchKernelGGL(gmres_dots_kernel<NV>, dim3(gd), dim3(kBlock), 0, st, N,  \
                     w, V + static_cast<size_t>(k0) * N,                      \
                     static_cast<size_t>(N), k0 == 0 ? 1 : 0,                 \
                     P + k0 * kRedBlocks, Pww, stop)
    FLOW_NV_SWITCH(chunk, FLOW_CALL)
#undef FLOW_CALL
  }
}

// One GMRES cycle from iteration it0: at most m columns and maxit - it0.  The
// planner decides how many Arnoldi steps go out before the host looks at the
// state S again -- what is left of `expected`, then one at a time, never past
// the room: the cycle makes progress towards maxit whatever the device
// reports -- and enqueues them with arnoldi(column, last).  Behind every
// read-back: *cols = the columns that are final, *resid = the residual
// estimate, *done = S[kDone] (0: the room is used up; 1: converged on the
// estimate; 3: the cycle ended without a verdict; 4: the start itself passed,
// nothing was done -- only a solver whose cycles begin on the device sees it).
// Not a number: the message, *iters_host, *resid_host, FLOW_NOT_CONVERGED.
static int gmres_cycle(const char* solver, int m, int maxit, int it0,
                       int expected, const double* S, hipStream_t st,
                       const std::function<int(int, bool)>& arnoldi, int* cols,
                       double* resid, int* done, int* iters_host,
                       double* resid_host) {
  double state[kNumSlots];
  int enq = 0, rc;
  *cols = *done = 0;
  while (true) {
    const int room = (m < maxit - it0 ? m : maxit - it0) - enq;
    if (room <= 0) return FLOW_OK;
    int plan = expected - (it0 + enq);
    if (plan < 1) plan = 1;
    if (plan > room) plan = room;
    for (int k = 0; k < plan; ++k, ++enq) {
      const bool last = enq + 1 >= m || it0 + enq + 1 >= maxit;
      if ((rc = arnoldi(enq, last))) return rc;
    }
    if ((rc = read_state(S, state, st))) return rc;
    *cols = static_cast<int>(state[kConvIt]);
    if (state[kDone] == 2.0) {
      *iters_host = it0 + *cols;
      *resid_host = state[kRes2];
      set_error("%s broke down (NaN) at iteration %d", solver, it0 + *cols);
      return FLOW_NOT_CONVERGED;
    }
    *resid = state[kRes2];
    *done = static_cast<int>(state[kDone]);
    if (*done != 0) return FLOW_OK;
  }
}

// work: [reductions | V_0 .. V_m | Z_0 .. Z_{m-1} | sweep buffer | partials |
// device state]; Z_j = M^-1 V_j is kept, so that the update x += sum_j y_j Z_j
// needs no further preconditioner application (memory is not the scarce
// resource).  expected: operator applications the caller expects the solve to
// need (0: unknown) -- that many Arnoldi steps are enqueued before the host
// looks at the state for the first time, then one at a time; the result does
// not depend on it.
static int gmres(const flow_operator* A, const double* dinv, const flow_ilu* ilu,
                 const flow_pmg* pmg, const double* b, double* x, double rtol,
                 double atol, int maxit, int m, int x_is_zero, int expected,
                 int verify, double* work, int* iters_host, double* resid_host,
                 hipStream_t st) {
  const int N = op_size(A);
  double* partial = work;
  double* S = work + 3 * kRedBlocks;
  double* V = work + FLOW_REDUCE_WORK;
  double* Z = V + static_cast<size_t>(m + 1) * N;
  double* iwork = Z + static_cast<size_t>(m) * N;
  double* P = iwork + N;                    // (kGmresMax + 2) x kRedBlocks
  double* Pww = P + kGmresMax * kRedBlocks;
  double* Pnn = Pww + kRedBlocks;
  double* G = P + FLOW_GMRES_PARTIALS;      // device state of the cycle
  const double* stop = S + kDone;
  const int gv = grid_for(N);
  const int gd = grid_for(N, kBlock, kRedBlocks);
  int np = 0, rc;

  const double* jprm = nullptr;   // (set with the graphs below)
  // Z_j = M^-1 V_j (without a preconditioner Z_j is V_j itself)
  const bool precond = pmg || ilu || dinv;
  const double* Zbase = precond ? Z : V;
  auto precondition = [&](int j) -> int {
    const double* in = V + static_cast<size_t>(j) * N;
    double* out = Z + static_cast<size_t>(j) * N;
    if (pmg) return pmg_apply(pmg, in, out, st, stop);
    if (ilu) return ilu_apply(ilu, in, out, iwork, st, stop);
    if (dinv)
      hipLaunchKernelGGL(vmul_kernel, dim3(gv), dim3(kBlock), 0, st, N, 1.0, dinv,
                         in, out, stop);
    return FLOW_OK;
  };
  // Arnoldi step j of the cycle, enqueued without a read-back
  auto arnoldi = [&](int j, double beta, double target, bool last) -> int {
    int r;
    double* w = V + static_cast<size_t>(j + 1) * N;
    if ((r = precondition(j))) return r;
    if ((r = apply(A, Zbase + static_cast<size_t>(j) * N, w, st, nullptr, stop, 0,
                   0, jprm)))
      return r;
    arnoldi_dots(N, j, w, V, gd, P, Pww, stop, st);
    hipLaunchKernelGGL(gmres_step_kernel, dim3(1), dim3(kBlock), 0, st, gd, j,
                       last ? 1 : 0, beta, target, P, G, S);
    FLOW_CHECK_LAUNCH();
    // the next basis vector, in place on w (skipped by the flag when the step
    // kernel has just accepted the iterate; not needed behind the last column)
    if (!last &&
        (r = gmres_combine_dev(N, j + 1, G + kGCoef, G + kGCw, w, V, w, Pnn, false,
                               stop, st)))
      return r;
    return FLOW_OK;
  };

  // Arnoldi step j as a HIP graph where the launch rate bounds it
  // (graph_replay.hip): one graph per column and `last` flag; the step size
  // of a matrix-free Jacobian travels through device memory (G + kGJvp), so
  // the graphs survive the step-size controller
  const bool replay = replay_wanted(N, kReplayGmres);
  KeyHash base;
  if (replay) {
    base.pod(0x676dull);      // "gm"
    key_operator(base, A, true);
    base.pod(dinv).obj(ilu).obj(ilu ? ilu->plan : nullptr).obj(pmg);
    base.pod(work).pod(N).pod(m);
    if (A->kind == 3) {
      jprm = G + kGJvp;
      if ((rc = momentum_jvp_params(
               static_cast<const flow_momentum_jvp*>(A->matfree), G + kGJvp, st)))
        return rc;
    }
  }
  auto arnoldi_replayed = [&](int j, bool last) -> int {
    if (!replay) return arnoldi(j, -1.0, 0.0, last);
    KeyHash key = base;
    key.pod(j).pod(last);
    hipGraphExec_t graph = nullptr;
    int nodes = 0, r;
    if ((r = replay_prepare(key.h, kReplayGmres, st,
                            [&]() { return arnoldi(j, -1.0, 0.0, last); }, &graph,
                            &nodes)))
      return r;
    return graph ? replay_launch(graph, nodes, st) : arnoldi(j, -1.0, 0.0, last);
  };

  if ((rc = fill(kNumSlots, 0.0, S, st))) return rc;
  double resid = 0.0;
  int it = 0;
  bool first = true;
  bool claimed = false;     // the last cycle stopped on the residual estimate
  double state[kNumSlots];
  while (true) {
    // r0 = b - A x -> V_0; |r0|^2 (the first time also |b|^2) in block
    // partials; beta = |r0|, the target and the verdict on the start itself
    // are left ON THE DEVICE by gmres_begin_kernel: nothing is read back
    // before the cycle's Arnoldi steps are enqueued
    const bool b_is_r0 = x_is_zero && it == 0;
    if (b_is_r0) {
      hipLaunchKernelGGL(axpby_kernel, dim3(gv), dim3(kBlock), 0, st, N, 1.0, b,
                         0.0, V);
    } else {
      if ((rc = apply(A, x, iwork, st))) return rc;
      hipLaunchKernelGGL(residual_kernel, dim3(gv), dim3(kBlock), 0, st, N, b,
                         iwork,
                         static_cast<const double*>(nullptr), V,
                         static_cast<double*>(nullptr));
    }
    const int have_b2 = first && !b_is_r0;
    if ((rc = dots(N, have_b2 ? 2 : 1, V, V, b, b, V, V, partial, &np, st)))
      return rc;
    // behind a cycle that stopped on the least-squares ESTIMATE this is the
    // verification with the true residual b - A x (one operator application):
    // the one-pass Gram-Schmidt and a reduced-precision preconditioner can
    // leave the estimate below the target while the true residual stagnates
    // (seen in principle at rtol 1e-13, flow/heat.py's solves); within a
    // factor 10 of the target the iterate is accepted and the TRUE norm
    // reported, beyond it the solve goes on from here
    hipLaunchKernelGGL(gmres_begin_kernel, dim3(1), dim3(kBlock), 0, st, np,
                       have_b2, first ? 1 : 0, claimed ? 1 : 0, rtol, atol,
                       partial, S);
    if (have_b2)     // (a start vector was handed in: keep it only if it helps)
      hipLaunchKernelGGL(gmres_drop_start_kernel, dim3(gv), dim3(kBlock), 0, st,
                         N, S, b, V, x);
    FLOW_CHECK_LAUNCH();
    first = false;
    claimed = false;
    if (it >= maxit) {
      if ((rc = read_state(S, state, st))) return rc;
      resid = state[kBeta];
      if (state[kDone] == 4.0) break;
      *iters_host = it;
      *resid_host = resid;
      if (state[kDone] == 2.0) {
        set_error("GMRES broke down (NaN residual) at iteration %d", it);
      } else {
        set_error("GMRES did not converge in %d iterations: |r| = %.3e > %.3e",
                  it, resid, state[kTarget2]);
      }
      return FLOW_NOT_CONVERGED;
    }

    // one cycle: up to m columns; `cols` of them are known to be final
    int cols, done;
    if ((rc = gmres_cycle("GMRES", m, maxit, it, expected, S, st,
                          arnoldi_replayed, &cols, &resid, &done, iters_host,
                          resid_host)))
      return rc;
    if (done == 4) break;             // r0 itself passed: nothing was done
    const bool converged = done == 1;   // 3: verify with the true residual
    // (a cycle that ends without a final column counts as one iteration: the
    // loop makes progress towards maxit whatever the device reports)
    it += cols > 0 ? cols : 1;
    // x += sum_k y_k Z_k / nrm_k (coefficients left by the last step kernel
    // that ran); the flag is taken down first: it has done its work
    if ((rc = fill(1, 0.0, S + kDone, st))) return rc;
    if (cols > 0 &&
        (rc = gmres_combine_dev(N, cols, G + kGYc, nullptr, nullptr, Zbase, x,
                                nullptr, true, nullptr, st)))
      return rc;
    x_is_zero = 0;
    if (converged && !verify) break;
    claimed = converged;
    // restart from the true residual: verify a claimed convergence there, go
    // on otherwise (or report non-convergence)
  }
  *iters_host = it;
  *resid_host = resid;
  return FLOW_OK;
}

static int check_solver_args(const flow_operator* A, const double* b,
                             const double* x, double rtol, double atol,
                             int maxit, int check_every, int first_check,
                             const double* work, size_t work_len, size_t nvec,
                             const int* iters_host, const double* resid_host) {
  int rc = check_operator(A);
  if (rc) return rc;
  FLOW_REQUIRE(b && x && work && iters_host && resid_host, "solver pointers");
  FLOW_REQUIRE(rtol >= 0.0 && atol >= 0.0 && maxit >= 0 && check_every > 0 &&
                   first_check >= 0,
               "solver tolerances");
  FLOW_REQUIRE(work_len >= FLOW_REDUCE_WORK + nvec * (size_t)op_size(A),
               "solver workspace too small");
  return FLOW_OK;
}

// the arguments of flow_cg_solve and flow_cg_solve_guarded
static int check_cg_args(const flow_operator* A, const double* dinv,
                         const flow_coarse* coarse, const flow_mg* mg,
                         const double* b, const double* x, double rtol,
                         double atol, int maxit, int check_every,
                         int first_check, const double* work, size_t work_len,
                         const int* iters_host, const double* resid_host) {
  int rc = check_solver_args(A, b, x, rtol, atol, maxit, check_every,
                             first_check, work, work_len, 5, iters_host,
                             resid_host);
  if (rc) return rc;
  FLOW_REQUIRE(A->kind != 3, "CG: assembled (symmetric) operators only");
  if (coarse) {
    FLOW_REQUIRE(dinv != nullptr, "two-level preconditioner needs dinv");
    FLOW_REQUIRE(A->kind == 0, "two-level preconditioner: scalar operators");
    if ((rc = check_coarse(coarse, A->n))) return rc;
  }
  if (mg) {
    FLOW_REQUIRE(coarse == nullptr, "multigrid and two-level are exclusive");
    FLOW_REQUIRE(dinv != nullptr && A->kind == 0,
                 "multigrid preconditioner: scalar operators with dinv");
    if ((rc = check_mg(mg, A->n))) return rc;
    FLOW_REQUIRE(mg->nlevels >= 2, "multigrid: at least two levels");
  }
  FLOW_REQUIRE(work_len >= cg_work_len(A, coarse, mg),
               "solver workspace too small (FLOW_REDUCE_WORK + 5 N + SpMV "
               "workgroups + 2 [+ 2 lda] [+ 2 mg->Ps[0].nblocks])");
  FLOW_REQUIRE(reinterpret_cast<uintptr_t>(work) % 16 == 0,
               "solver workspace must be 16-byte aligned");
  return FLOW_OK;
}

extern "C" int flow_cg_solve(const flow_operator* A, const double* dinv,
                             const flow_coarse* coarse, const flow_mg* mg,
                             const double* b,
                             double* x, double rtol, double atol, int maxit,
                             int check_every, int first_check, double* work,
                             size_t work_len, int* iters_host,
                             double* resid_host, void* stream) {
  int rc = check_cg_args(A, dinv, coarse, mg, b, x, rtol, atol, maxit,
                         check_every, first_check, work, work_len, iters_host,
                         resid_host);
  if (rc) return rc;
  return cg(A, dinv, coarse, mg, b, x, rtol, atol, maxit, check_every,
            first_check, work, iters_host, resid_host, as_stream(stream));
}

// The same solve from a GUARDED start vector: a start that leaves a larger
// preconditioned residual than x = 0 would (|B(b - A x)| > |B b|, decided on
// the device from the numbers the first iteration forms anyway) is dropped
// for `x_fallback` (guarded as well; NULL: none), and that for zero -- the
// reference's start (a fresh Function, pressure_correction.py:313).
extern "C" int flow_cg_solve_guarded(
    const flow_operator* A, const double* dinv, const flow_coarse* coarse,
    const flow_mg* mg, const double* b, double* x, const double* x_fallback,
    double rtol, double atol, int maxit, int check_every, int first_check,
    double* work, size_t work_len, int* iters_host, double* resid_host,
    int* starts_dropped_host, void* stream) {
  FLOW_REQUIRE(starts_dropped_host != nullptr, "starts_dropped_host is NULL");
  *starts_dropped_host = 0;
  int rc = check_cg_args(A, dinv, coarse, mg, b, x, rtol, atol, maxit,
                         check_every, first_check, work, work_len, iters_host,
                         resid_host);
  if (rc) return rc;
  FLOW_REQUIRE(x_fallback != x, "the fallback start must not alias x");
  hipStream_t st = as_stream(stream);
  const int N = op_size(A);
  bool rejected = false;
  rc = cg(A, dinv, coarse, mg, b, x, rtol, atol, maxit, check_every,
          first_check, work, iters_host, resid_host, st, &rejected);
  if (rc || !rejected) return rc;
  *starts_dropped_host = 1;
  if (x_fallback) {
    hipLaunchKernelGGL(axpby_kernel, dim3(grid_for(N)), dim3(kBlock), 0, st, N,
                       1.0, x_fallback, 0.0, x);
    FLOW_CHECK_LAUNCH();
    rc = cg(A, dinv, coarse, mg, b, x, rtol, atol, maxit, check_every, 0, work,
            iters_host, resid_host, st, &rejected);
    if (rc || !rejected) return rc;
    *starts_dropped_host = 2;
  }
  if ((rc = fill(N, 0.0, x, st))) return rc;
  return cg(A, dinv, coarse, mg, b, x, rtol, atol, maxit, check_every, 0, work,
            iters_host, resid_host, st);
}

// z = V-cycle(r): one application of the multigrid preconditioner (tests, and
// callers that drive their own Krylov loop)
extern "C" int flow_mg_apply(const flow_mg* mg, int n, const double* r,
                             double* z, void* stream) {
  FLOW_REQUIRE(mg && r && z && r != z && n > 0, "mg apply");
  int rc = check_mg(mg, n);
  if (rc) return rc;
  return vcycle(mg, r, z, as_stream(stream));
}

// z = D^-1 r + P Ac^-1 P^T r: one application of the two-level preconditioner
// (callers that drive their own Krylov loop: the Stokes MINRES)
extern "C" int flow_two_level_apply(const flow_coarse* coarse,
                                    const double* dinv, const double* r,
                                    double* z, double* work, void* stream) {
  FLOW_REQUIRE(coarse && dinv && r && z && work && r != z, "two-level apply");
  int rc = check_coarse(coarse, coarse->n);
  if (rc) return rc;
  FLOW_REQUIRE(reinterpret_cast<uintptr_t>(work) % 16 == 0,
               "two-level workspace must be 16-byte aligned");
  return two_level(coarse, dinv, r, z, work, work + coarse->lda,
                   as_stream(stream));
}

extern "C" int flow_bicgstab_solve(const flow_operator* A, const double* dinv,
                                   const flow_ilu* ilu, const double* b,
                                   double* x, double rtol, double atol,
                                   int maxit, int check_every,
                                   int first_check, double* work,
                                   size_t work_len, int* iters_host,
                                   double* resid_host, void* stream) {
  int rc = check_solver_args(A, b, x, rtol, atol, maxit, check_every,
                             first_check, work, work_len, 7, iters_host,
                             resid_host);
  if (rc) return rc;
  if (ilu) {
    if ((rc = ilu_check(ilu, op_size(A)))) return rc;
    FLOW_REQUIRE(work_len >= FLOW_REDUCE_WORK + 8 * (size_t)op_size(A),
                 "solver workspace too small for the ILU sweep buffer");
  }
  return bicgstab(A, dinv, ilu, b, x, rtol, atol, maxit, check_every,
                  first_check, work, iters_host, resid_host, as_stream(stream));
}

int flow::check_gmres_args(int restart, int expected_its) {
  FLOW_REQUIRE(restart >= 1 && restart <= FLOW_GMRES_MAX_RESTART,
               "GMRES restart length");
  FLOW_REQUIRE(expected_its >= 0, "expected iterations");
  return FLOW_OK;
}

extern "C" int flow_gmres_solve(const flow_operator* A, const double* dinv,
                                const flow_ilu* ilu, const flow_pmg* pmg,
                                const double* b, double* x,
                                double rtol, double atol, int maxit, int restart,
                                int x_is_zero, int expected_its, int verify,
                                double* work, size_t work_len, int* iters_host,
                                double* resid_host, void* stream) {
  int rc = check_solver_args(A, b, x, rtol, atol, maxit, 1, 0, work, work_len, 0,
                             iters_host, resid_host);
  if (rc || (rc = check_gmres_args(restart, expected_its))) return rc;
  FLOW_REQUIRE(work_len >= FLOW_REDUCE_WORK +
                               (2 * static_cast<size_t>(restart) + 2) *
                                   op_size(A) +
                               FLOW_GMRES_PARTIALS + FLOW_GMRES_STATE,
               "solver workspace too small (FLOW_REDUCE_WORK + (2 restart + 2) N "
               "+ FLOW_GMRES_PARTIALS + FLOW_GMRES_STATE)");
  FLOW_REQUIRE(!(ilu && pmg), "one preconditioner: ilu or pmg");
  if (ilu && (rc = ilu_check(ilu, op_size(A)))) return rc;
  if (pmg && (rc = pmg_check(pmg, op_size(A)))) return rc;
  return gmres(A, dinv, ilu, pmg, b, x, rtol, atol, maxit, restart, x_is_zero,
               expected_its, verify, work, iters_host, resid_host,
               as_stream(stream));
}
