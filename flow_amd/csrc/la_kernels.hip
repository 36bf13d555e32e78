// Sparse linear algebra of the hot path on gfx950: CSR-stream SpMV (K8), fused
// BLAS-1 (K9), Jacobi (K10), the read-backs and the small vector utilities.
// The device-resident Krylov drivers (K12) built on them: krylov_kernels.hip;
// the domain decomposition (K15): shard_kernels.hip; what the units share:
// la_internal.h.
//
// Replaces PETSc MatMult / VecDot / VecAXPY / KSPCG inside dolfin's `solve`
// (reference: flow/navier_stokes/pressure_correction.py:326-339, 419-432,
// 451-464) and the `M * uvec`, `A * uvec` products of flow/heat.py:101.
//
// All kernels are HBM-bandwidth bound (0.17 flop/B); no MFMA.  Design:
//  * SpMV = CSR-stream: a 256-thread workgroup owns a block of <=256 consecutive
//    rows holding <=2048 nonzeros.  Phase 1 streams vals/cols fully coalesced
//    (every lane busy, independent of the row length ~7) and parks the
//    products a_ij*x_j in LDS; phase 2 is the segmented reduction: one lane per
//    row sums its LDS segment [rowptr[r], rowptr[r+1]) -- odd row lengths make
//    the LDS reads bank-conflict free -- and stores y coalesced.
//  * reductions never use fp atomics: <=1024 per-block partials + a one-block
//    finisher => bitwise reproducible.
//  * Krylov scalars (alpha, beta, ...) live in HBM; the host only reads the
//    residual norm every `check_every` iterations.
#include "common.h"
#include "csr_stream.h"
#include "la_internal.h"

namespace flow {

thread_local char g_error[512] = "";

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_error, sizeof(g_error), fmt, ap);
  va_end(ap);
}

// ---------------------------------------------------------------------------
// Krylov: scalar slots in HBM
// ---------------------------------------------------------------------------
// (enum Slot: common.h)
// (the scalars move with load_scalar / store_scalar: common.h)
// work layout: [0, 3*kRedBlocks) partials, [3*kRedBlocks, +kNumSlots) scalars
static_assert(3 * kRedBlocks + kNumSlots <= FLOW_REDUCE_WORK, "work size");

// Convergence is decided ON THE DEVICE: the kernel that computes the solver
// scalars compares the (preconditioned) residual with the target, and from the first iterate that passes
// the test on sets the sticky flag S[kDone] (1 converged, 2 breakdown); every
// kernel of the iteration body takes `stop` = S + kDone and returns at once
// when it is set.  The host can therefore enqueue iterations ahead of its
// read-backs without the solution moving past the iterate the stopping test
// accepted (running CG on after its recurrence residual has reached rounding
// level is not harmless: measured on the P2 mass matrix, 8 iterations past
// convergence moved the solution by 1.8e-4 relative), and the iteration count
// it reports is the exact one.
// (stopped(): common.h)

// ---------------------------------------------------------------------------
// SpMV
// ---------------------------------------------------------------------------
// (tiles: csr_stream.h)
// scalar plane(s): blockIdx.y selects the component of a block-diagonal operator.
// DOT: the workgroup also leaves its share of x.y (= x.Ax) in
// dpart[blockIdx.y * gridDim.x + blockIdx.x] (CG's z.w without another pass).
template <bool DOT>
__global__ __launch_bounds__(kBlock) void spmv_stream_kernel(
    int n, const int* __restrict__ rowptr, const int* __restrict__ cols,
    const double* __restrict__ vals0, const double* __restrict__ vals1,
    const int* __restrict__ rowblocks, const double* __restrict__ x,
    double* __restrict__ y, double* __restrict__ dpart,
    const double* __restrict__ stop) {
  __shared__ double prod[kTile];
  if (stopped(stop)) return;
  const double* __restrict__ vals = blockIdx.y == 0 ? vals0 : vals1;
  x += static_cast<size_t>(blockIdx.y) * n;
  y += static_cast<size_t>(blockIdx.y) * n;
  int r, r1;
  double xi = 0.0;
  auto early = [&](int row, bool has) {
    if (DOT && has) xi = x[row];
  };
  const double s =
      stream_tile_row_sum(rowptr, cols, vals, rowblocks, x, prod, r, r1, early);
  double t = 0.0;
  if (r < r1) {
    y[r] = s;
    if (DOT) t = s * xi;
  }
  if (DOT) {
    t = block_sum_once(t);
    if (threadIdx.x == 0) dpart[blockIdx.y * gridDim.x + blockIdx.x] = t;
  }
}

// full 2x2 blocks over one scalar pattern (Newton Jacobian)
template <bool DOT>
__global__ __launch_bounds__(kBlock) void spmv_stream_block2_kernel(
    int n, const int* __restrict__ rowptr, const int* __restrict__ cols,
    const double* __restrict__ vxx, const double* __restrict__ vxy,
    const double* __restrict__ vyx, const double* __restrict__ vyy,
    const int* __restrict__ rowblocks, const double* __restrict__ x,
    double* __restrict__ y, double* __restrict__ dpart,
    const double* __restrict__ stop) {
  __shared__ double prod0[kTile2];
  __shared__ double prod1[kTile2];
  if (stopped(stop)) return;
  const int tile = xcd_tile(blockIdx.x, gridDim.x);
  const int r0 = rowblocks[tile];
  const int r1 = rowblocks[tile + 1];
  const int k0 = rowptr[r0];
  const int k1 = rowptr[r1];
  const int ka = k0 & ~1;
  const int r = r0 + threadIdx.x;
  int a = 0, b = 0;
  if (r < r1) {
    a = rowptr[r] - ka;
    b = rowptr[r + 1] - ka;
  }
  const int npair = (k1 - ka + 1) >> 1;
  const int2* __restrict__ c2p = reinterpret_cast<const int2*>(cols + ka);
  const double2* __restrict__ pxx = reinterpret_cast<const double2*>(vxx + ka);
  const double2* __restrict__ pxy = reinterpret_cast<const double2*>(vxy + ka);
  const double2* __restrict__ pyx = reinterpret_cast<const double2*>(vyx + ka);
  const double2* __restrict__ pyy = reinterpret_cast<const double2*>(vyy + ka);
#pragma unroll
  for (int j = 0; j < kPairs2; ++j) {
    const int p = threadIdx.x + j * kBlock;
    if (p < npair) {
      const int2 c = c2p[p];
      const double2 axx = pxx[p], axy = pxy[p], ayx = pyx[p], ayy = pyy[p];
      // (only the tile's own columns are dereferenced)
      const int cx = 2 * p >= k0 - ka ? c.x : cols[k0];
      const int cy = 2 * p + 1 < k1 - ka ? c.y : cols[k0];
      const double u0 = x[cx], u1 = x[n + cx];
      const double w0 = x[cy], w1 = x[n + cy];
      prod0[2 * p] = axx.x * u0 + axy.x * u1;
      prod1[2 * p] = ayx.x * u0 + ayy.x * u1;
      prod0[2 * p + 1] = axx.y * w0 + axy.y * w1;
      prod1[2 * p + 1] = ayx.y * w0 + ayy.y * w1;
    }
  }
  __syncthreads();
  double t = 0.0;
  if (r < r1) {
    double s0 = 0.0, s1 = 0.0;
    for (int k = a; k < b; ++k) {
      s0 += prod0[k];
      s1 += prod1[k];
    }
    y[r] = s0;
    y[n + r] = s1;
    if (DOT) t = s0 * x[r] + s1 * x[n + r];
  }
  if (DOT) {
    t = block_sum_once(t);
    if (threadIdx.x == 0) dpart[blockIdx.x] = t;
  }
}

// one value plane applied to both components of a component-blocked vector,
// identity on the rows with mask 0 (flow_operator kind 4): the matrix is read
// once for the two products
template <bool DOT>
__global__ __launch_bounds__(kBlock) void spmv_stream_pair_kernel(
    int n, const int* __restrict__ rowptr, const int* __restrict__ cols,
    const double* __restrict__ vals, const int* __restrict__ rowblocks,
    const unsigned char* __restrict__ mask, const double* __restrict__ x,
    double* __restrict__ y, int xs, double* __restrict__ dpart,
    const double* __restrict__ stop) {
  // (the tile: stream_tile_pair_row_sum, csr_stream.h)
  __shared__ double2 prod[kTile2];
  if (stopped(stop)) return;
  int r, r1;
  const double2 s =
      stream_tile_pair_row_sum(rowptr, cols, vals, rowblocks, x, xs, prod, r, r1);
  double s0 = s.x, s1 = s.y;
  double t = 0.0;
  if (r < r1) {
    const double x0 = x[r], x1 = x[xs + r];
    if (!mask[r]) s0 = x0;
    if (!mask[n + r]) s1 = x1;
    y[r] = s0;
    y[xs + r] = s1;
    if (DOT) t = s0 * x0 + s1 * x1;
  }
  if (DOT) {
    t = block_sum_once(t);
    if (threadIdx.x == 0) dpart[blockIdx.x] = t;
  }
}

int check_operator(const flow_operator* A) {
  FLOW_REQUIRE(A != nullptr, "operator is NULL");
  FLOW_REQUIRE(A->kind >= 0 && A->kind <= 4, "operator kind");
  if (A->kind == 3) {   // matrix-free: no pattern, no value planes
    const flow_momentum_jvp* J =
        static_cast<const flow_momentum_jvp*>(A->matfree);
    int rc = momentum_jvp_check(J);
    if (rc) return rc;
    FLOW_REQUIRE(A->n == J->W->n, "matrix-free operator size");
    return FLOW_OK;
  }
  FLOW_REQUIRE(A->n > 0 && A->nnz > 0 && A->nblocks > 0, "operator sizes");
  FLOW_REQUIRE(A->rowptr && A->cols && A->rowblocks, "operator pattern");
  const int planes = (A->kind == 0 || A->kind == 4) ? 1 : (A->kind == 1 ? 2 : 4);
  FLOW_REQUIRE(A->kind != 4 || A->rowmask != nullptr, "operator row mask");
  for (int p = 0; p < planes; ++p) {
    FLOW_REQUIRE(A->vals[p] != nullptr, "operator value plane");
    FLOW_REQUIRE((reinterpret_cast<size_t>(A->vals[p]) & 15) == 0,
                 "value planes must be 16-byte aligned");
  }
  FLOW_REQUIRE((reinterpret_cast<size_t>(A->cols) & 7) == 0,
               "cols must be 8-byte aligned");
  return FLOW_OK;
}

// (op_size, dot_parts, SpmvProfile: la_internal.h)
SpmvProfile g_spmv_profile;

// every value of an operator that reaches a kernel (graph_replay.hip)
void key_operator(KeyHash& k, const flow_operator* A, bool skip_prm) {
  k.obj(A);
  if (A && A->kind == 3 && A->matfree) {
    flow_momentum_jvp J = *static_cast<const flow_momentum_jvp*>(A->matfree);
    if (skip_prm) J.prm = flow_ns_params{0.0, 0.0, 0.0, 0.0, 0.0};
    k.obj(&J).obj(J.mesh).obj(J.W);
  }
}

// y = A x [and the shares of x.y]: see la_internal.h
int apply(const flow_operator* A, const double* x, double* y, hipStream_t st,
          double* dpart, const double* stop, int vec_stride, int out_stride,
          const double* jvp_prm) {
  if (A->kind == 3) {
    FLOW_REQUIRE(dpart == nullptr, "matrix-free operators carry no fused dot");
    return momentum_jvp_apply(static_cast<const flow_momentum_jvp*>(A->matfree),
                              x, y, st, vec_stride, out_stride, stop, jvp_prm);
  }
  const int xs = vec_stride ? vec_stride : A->n;
  const dim3 grid(A->nblocks, A->kind == 1 ? 2 : 1);
  const double* v1 = A->kind == 1 ? A->vals[1] : A->vals[0];
  if (A->kind == 4) {
    if (dpart)
      hipLaunchKernelGGL(spmv_stream_pair_kernel<true>, grid, dim3(kBlock), 0, st,
                         A->n, A->rowptr, A->cols, A->vals[0], A->rowblocks,
                         A->rowmask, x, y, xs, dpart, stop);
    else
      hipLaunchKernelGGL(spmv_stream_pair_kernel<false>, grid, dim3(kBlock), 0,
                         st, A->n, A->rowptr, A->cols, A->vals[0], A->rowblocks,
                         A->rowmask, x, y, xs, dpart, stop);
  } else if (A->kind == 2) {
    if (dpart)
      hipLaunchKernelGGL(spmv_stream_block2_kernel<true>, grid, dim3(kBlock), 0,
                         st, A->n, A->rowptr, A->cols, A->vals[0], A->vals[1],
                         A->vals[2], A->vals[3], A->rowblocks, x, y, dpart,
                         stop);
    else
      hipLaunchKernelGGL(spmv_stream_block2_kernel<false>, grid, dim3(kBlock), 0,
                         st, A->n, A->rowptr, A->cols, A->vals[0], A->vals[1],
                         A->vals[2], A->vals[3], A->rowblocks, x, y, dpart,
                         stop);
  } else if (dpart) {
    SpmvProfile& pf = g_spmv_profile;
    const bool timed = pf.used < pf.cap && A->kind == 0 && A->n == pf.rows;
    if (timed) FLOW_CHECK_HIP(hipEventRecord(pf.ev[2 * pf.used], st));
    hipLaunchKernelGGL(spmv_stream_kernel<true>, grid, dim3(kBlock), 0, st, A->n,
                       A->rowptr, A->cols, A->vals[0], v1, A->rowblocks, x, y,
                       dpart, stop);
    if (timed) FLOW_CHECK_HIP(hipEventRecord(pf.ev[2 * pf.used++ + 1], st));
  } else {
    hipLaunchKernelGGL(spmv_stream_kernel<false>, grid, dim3(kBlock), 0, st,
                       A->n, A->rowptr, A->cols, A->vals[0], v1, A->rowblocks, x,
                       y, dpart, stop);
  }
  FLOW_CHECK_LAUNCH();
  return FLOW_OK;
}

int operator_apply(const flow_operator* A, const double* x, double* y,
                   hipStream_t st, const double* stop) {
  return apply(A, x, y, st, nullptr, stop);
}
int operator_size(const flow_operator* A) { return op_size(A); }

__global__ void diag_inv_kernel(int n, int planes_kind,
                                const int* __restrict__ diag_idx,
                                const double* __restrict__ v0,
                                const double* __restrict__ v1,
                                const unsigned char* __restrict__ mask,
                                double* __restrict__ dinv) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += gridDim.x * blockDim.x) {
    const int k = diag_idx[i];
    dinv[i] = (mask && !mask[i]) ? 1.0 : 1.0 / v0[k];
    if (planes_kind > 0)
      dinv[n + i] = (mask && !mask[n + i]) ? 1.0 : 1.0 / v1[k];
  }
}

// ---------------------------------------------------------------------------
// BLAS-1
// ---------------------------------------------------------------------------
// up to three dot products in one pass; partial[j*kRedBlocks + block]
__global__ __launch_bounds__(kBlock) void dot3_kernel(
    int n, int nd, const double* __restrict__ a0, const double* __restrict__ b0,
    const double* __restrict__ a1, const double* __restrict__ b1,
    const double* __restrict__ a2, const double* __restrict__ b2,
    double* __restrict__ partial) {
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += gridDim.x * blockDim.x) {
    s0 += a0[i] * b0[i];
    if (nd > 1) s1 += a1[i] * b1[i];
    if (nd > 2) s2 += a2[i] * b2[i];
  }
  s0 = block_sum(s0);
  if (nd > 1) s1 = block_sum(s1);
  if (nd > 2) s2 = block_sum(s2);
  if (threadIdx.x == 0) {
    partial[blockIdx.x] = s0;
    if (nd > 1) partial[kRedBlocks + blockIdx.x] = s1;
    if (nd > 2) partial[2 * kRedBlocks + blockIdx.x] = s2;
  }
}

__global__ __launch_bounds__(kBlock) void absmax_kernel(
    int n, const double* __restrict__ x, double* __restrict__ partial) {
  double m = 0.0;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += gridDim.x * blockDim.x)
    m = fmax(m, fabs(x[i]));
  m = block_max(m);
  if (threadIdx.x == 0) partial[blockIdx.x] = m;
}

// one block: out[j] = reduce(partial[j*kRedBlocks .. +nparts)), fixed order
__global__ __launch_bounds__(kBlock) void finish_kernel(
    int nparts, int nd, int is_max, const double* __restrict__ partial,
    double* __restrict__ out) {
  for (int j = 0; j < nd; ++j) {
    double v = 0.0;
    for (int i = threadIdx.x; i < nparts; i += kBlock) {
      const double p = load_scalar(partial + j * kRedBlocks + i);
      v = is_max ? fmax(v, p) : v + p;
    }
    v = is_max ? block_max(v) : block_sum(v);
    if (threadIdx.x == 0) store_scalar(out + j, v);
  }
}

__global__ void axpby_kernel(int n, double a, const double* __restrict__ x,
                             double b, double* __restrict__ y) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += gridDim.x * blockDim.x)
    y[i] = (b == 0.0) ? a * x[i] : a * x[i] + b * y[i];
}

// y = value.  Fills and copies of the solvers are plain kernels of the stream
// (not hipMemsetAsync / hipMemcpyAsync): measured on MI355X with several
// processes sharing the GPU, the runtime's copy operations were not always
// ordered against the neighbouring kernels of the same stream (BiCGStab's
// shadow residual rhat = r0 was copied after r had already been updated).
__global__ void fill_kernel(int n, double value, double* __restrict__ y) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += gridDim.x * blockDim.x)
    y[i] = value;
}

int fill(int n, double value, double* y, hipStream_t st) {
  hipLaunchKernelGGL(fill_kernel, dim3(grid_for(n)), dim3(kBlock), 0, st, n,
                     value, y);
  FLOW_CHECK_LAUNCH();
  return FLOW_OK;
}

// out = a * x .* y  (masks, diagonal scalings; out may alias x or y)
__global__ void vmul_kernel(int n, double a, const double* x, const double* y,
                            double* out, const double* stop) {
  if (stopped(stop)) return;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += gridDim.x * blockDim.x)
    out[i] = a * x[i] * y[i];
}

// r = b - q ; z = dinv*r
__global__ void residual_kernel(int n, const double* __restrict__ b,
                                const double* __restrict__ q,
                                const double* __restrict__ dinv,
                                double* __restrict__ r, double* __restrict__ z) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += gridDim.x * blockDim.x) {
    const double ri = b[i] - q[i];
    r[i] = ri;
    if (z) z[i] = dinv ? dinv[i] * ri : ri;
  }
}

int dots(int n, int nd, const double* a0, const double* b0, const double* a1,
         const double* b1, const double* a2, const double* b2, double* partial,
         int* nparts, hipStream_t st) {
  const int g = grid_for(n, kBlock * 4, kRedBlocks);
  hipLaunchKernelGGL(dot3_kernel, dim3(g), dim3(kBlock), 0, st, n, nd, a0, b0,
                     a1, b1, a2, b2, partial);
  FLOW_CHECK_LAUNCH();
  *nparts = g;
  return FLOW_OK;
}

// The stream is drained BEFORE the copy is issued as well: measured on MI355X
// with several processes sharing the GPU, a small device-to-host copy into
// pageable memory enqueued right behind kernels of the same stream did not
// always see their results (stale residual norms => different, though equally
// valid, stopping iterations from one process to the next).
//
// Read-backs therefore do not use the runtime's copy at all: a one-thread
// kernel of the same stream stores the scalar into host-coherent (pinned,
// mapped) memory with a system-scope fence, the host waits for the stream and
// reads it.  The mailbox (a few doubles per host thread) is the only memory
// the library ever allocates.
__global__ void mailbox_kernel(const double* __restrict__ src0,
                               const double* __restrict__ src1,
                               volatile double* __restrict__ mailbox) {
  mailbox[0] = load_scalar(src0);
  mailbox[1] = load_scalar(src1);
  __threadfence_system();
}

// the calling thread's mailbox: kMailbox doubles of pinned, mapped host memory
static int mailbox_of_thread(double** host, double** dev) {
  static thread_local double* mailbox = nullptr;
  if (!mailbox)
    FLOW_CHECK_HIP(hipHostMalloc(reinterpret_cast<void**>(&mailbox),
                                 kMailbox * sizeof(double), hipHostMallocMapped));
  *host = mailbox;
  FLOW_CHECK_HIP(
      hipHostGetDevicePointer(reinterpret_cast<void**>(dev), mailbox, 0));
  return FLOW_OK;
}

// two scalars of the stream's device memory -> host, with ONE synchronisation
static int read_slots(const double* S, int slot0, int slot1, double* host0,
                      double* host1, hipStream_t st) {
  double *mailbox = nullptr, *dev_view = nullptr;
  int rc = mailbox_of_thread(&mailbox, &dev_view);
  if (rc) return rc;
  hipLaunchKernelGGL(mailbox_kernel, dim3(1), dim3(1), 0, st, S + slot0,
                     S + slot1, dev_view);
  FLOW_CHECK_LAUNCH();
  FLOW_CHECK_HIP(hipStreamSynchronize(st));
  *host0 = static_cast<volatile double*>(mailbox)[0];
  *host1 = static_cast<volatile double*>(mailbox)[1];
  return FLOW_OK;
}

// all the solver scalars S[0, kNumSlots) -> host (one synchronisation)
__global__ void mailbox_state_kernel(const double* __restrict__ S,
                                     volatile double* __restrict__ mailbox) {
  if (threadIdx.x < kNumSlots) mailbox[threadIdx.x] = load_scalar(S + threadIdx.x);
  __threadfence_system();
}

int read_state(const double* S, double* host, hipStream_t st) {
  double *mailbox = nullptr, *dev_view = nullptr;
  int rc = mailbox_of_thread(&mailbox, &dev_view);
  if (rc) return rc;
  hipLaunchKernelGGL(mailbox_state_kernel, dim3(1), dim3(64), 0, st, S, dev_view);
  FLOW_CHECK_LAUNCH();
  FLOW_CHECK_HIP(hipStreamSynchronize(st));
  for (int i = 0; i < kNumSlots; ++i)
    host[i] = static_cast<volatile double*>(mailbox)[i];
  return FLOW_OK;
}

static int read_slot(const double* S, int slot, double* host, hipStream_t st) {
  double again;
  return read_slots(S, slot, slot, host, &again, st);
}

// sum of the first nparts (<= kRedBlocks) block partials at the head of a
// FLOW_REDUCE_WORK buffer, read back to the host (pmg_kernels.hip: the power
// iteration of the Chebyshev setup)
int sum_partials_host(double* work, int nparts, double* host, hipStream_t st) {
  FLOW_REQUIRE(nparts >= 1 && nparts <= kRedBlocks, "partial count");
  double* S = work + 3 * kRedBlocks;
  hipLaunchKernelGGL(finish_kernel, dim3(1), dim3(kBlock), 0, st, nparts, 1, 0,
                     work, S);
  FLOW_CHECK_LAUNCH();
  return read_slot(S, 0, host, st);
}

// n doubles of device memory -> the host mailbox
__global__ void mailbox_copy_kernel(int n, const double* __restrict__ src,
                                    volatile double* __restrict__ mailbox) {
  if (threadIdx.x < n) mailbox[threadIdx.x] = load_scalar(src + threadIdx.x);
  __threadfence_system();
}

int read_values(const double* dev, int n, double* host, hipStream_t st) {
  double *mailbox = nullptr, *dev_view = nullptr;
  int rc = mailbox_of_thread(&mailbox, &dev_view);
  if (rc) return rc;
  FLOW_REQUIRE(n <= kMailbox, "mailbox size");
  hipLaunchKernelGGL(mailbox_copy_kernel, dim3(1), dim3(64), 0, st, n, dev,
                     dev_view);
  FLOW_CHECK_LAUNCH();
  FLOW_CHECK_HIP(hipStreamSynchronize(st));
  for (int i = 0; i < n; ++i) host[i] = static_cast<volatile double*>(mailbox)[i];
  return FLOW_OK;
}

}  // namespace flow

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
using namespace flow;

extern "C" const char* flow_last_error(void) { return g_error; }
extern "C" int flow_abi_version(void) { return 30; }

namespace flow {
unsigned long long g_launches = 0;
}
extern "C" int flow_launch_count(unsigned long long* count_host) {
  FLOW_REQUIRE(count_host != nullptr, "flow_launch_count argument");
  *count_host = flow::g_launches;
  return FLOW_OK;
}

// n <= 64 doubles of device memory -> the host, in stream order (one
// synchronisation through the calling thread's mailbox)
extern "C" int flow_read_doubles(const double* dev, int n, double* host,
                                 void* stream) {
  FLOW_REQUIRE(dev && host && n >= 1 && n <= flow::kMailbox,
               "read_doubles arguments (1..64 values)");
  return flow::read_values(dev, n, host, flow::as_stream(stream));
}

extern "C" int flow_operator_apply(const flow_operator* A, const double* x,
                                   double* y, void* stream) {
  int rc = check_operator(A);
  if (rc) return rc;
  FLOW_REQUIRE(x && y && x != y, "x, y");
  return apply(A, x, y, as_stream(stream));
}

extern "C" int flow_operator_diag_inv(const flow_operator* A,
                                      const int* diag_idx, double* dinv,
                                      void* stream) {
  int rc = check_operator(A);
  if (rc) return rc;
  FLOW_REQUIRE(diag_idx && dinv, "diag_idx, dinv");
  FLOW_REQUIRE(A->kind != 3, "a matrix-free operator has no stored diagonal");
  const double* v1 = (A->kind == 0 || A->kind == 4)
                         ? A->vals[0]
                         : (A->kind == 1 ? A->vals[1] : A->vals[3]);
  hipLaunchKernelGGL(diag_inv_kernel, dim3(grid_for(A->n)), dim3(kBlock), 0,
                     as_stream(stream), A->n, A->kind, diag_idx, A->vals[0], v1,
                     A->kind == 4 ? A->rowmask
                                  : static_cast<const unsigned char*>(nullptr),
                     dinv);
  FLOW_CHECK_LAUNCH();
  return FLOW_OK;
}

// vals[k] *= d[row of k]: row equilibration of a scalar CSR plane (a Krylov
// residual test needs balanced rows: flow_amd/heat.py)
__global__ void scale_rows_kernel(int n, const int* __restrict__ rowptr,
                                  const double* __restrict__ d,
                                  double* __restrict__ vals) {
  for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < n;
       r += gridDim.x * blockDim.x) {
    const double di = d[r];
    for (int k = rowptr[r]; k < rowptr[r + 1]; ++k) vals[k] *= di;
  }
}

extern "C" int flow_scale_rows(int n, const int* rowptr, const double* d,
                               double* vals, void* stream) {
  FLOW_REQUIRE(n > 0 && rowptr && d && vals, "scale rows arguments");
  hipLaunchKernelGGL(scale_rows_kernel, dim3(grid_for(n)), dim3(kBlock), 0,
                     as_stream(stream), n, rowptr, d, vals);
  FLOW_CHECK_LAUNCH();
  return FLOW_OK;
}

extern "C" int flow_dot_host(int n, const double* x, const double* y,
                             double* work, double* result_host, void* stream) {
  FLOW_REQUIRE(n > 0 && x && y && work && result_host, "dot arguments");
  hipStream_t st = as_stream(stream);
  int np = 0;
  int rc = dots(n, 1, x, y, x, y, x, y, work, &np, st);
  if (rc) return rc;
  double* S = work + 3 * kRedBlocks;
  hipLaunchKernelGGL(finish_kernel, dim3(1), dim3(kBlock), 0, st, np, 1, 0, work,
                     S);
  FLOW_CHECK_LAUNCH();
  return read_slot(S, 0, result_host, st);
}

extern "C" int flow_norm_host(int n, const double* x, int kind, double* work,
                              double* result_host, void* stream) {
  FLOW_REQUIRE(n > 0 && x && work && result_host, "norm arguments");
  FLOW_REQUIRE(kind == 0 || kind == 1, "norm kind");
  hipStream_t st = as_stream(stream);
  double* S = work + 3 * kRedBlocks;
  if (kind == 0) {
    int rc = flow_dot_host(n, x, x, work, result_host, stream);
    if (rc) return rc;
    *result_host = sqrt(*result_host);
    return FLOW_OK;
  }
  const int g = grid_for(n, kBlock * 4, kRedBlocks);
  hipLaunchKernelGGL(absmax_kernel, dim3(g), dim3(kBlock), 0, st, n, x, work);
  hipLaunchKernelGGL(finish_kernel, dim3(1), dim3(kBlock), 0, st, g, 1, 1, work,
                     S);
  FLOW_CHECK_LAUNCH();
  return read_slot(S, 0, result_host, st);
}

extern "C" int flow_axpby(int n, double a, const double* x, double b, double* y,
                          void* stream) {
  FLOW_REQUIRE(n > 0 && x && y, "axpby arguments");
  hipLaunchKernelGGL(axpby_kernel, dim3(grid_for(n)), dim3(kBlock), 0,
                     as_stream(stream), n, a, x, b, y);
  FLOW_CHECK_LAUNCH();
  return FLOW_OK;
}

// dst[a*dst_stride + k] = src[a*src_stride + idx[k]]
__global__ void gather_rows_kernel(int ncomp, int m, const int* __restrict__ idx,
                                   const double* __restrict__ src, int src_stride,
                                   double* __restrict__ dst, int dst_stride) {
  for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < ncomp * m;
       t += gridDim.x * blockDim.x) {
    const int a = t / m, k = t - a * m;
    dst[static_cast<size_t>(a) * dst_stride + k] =
        src[static_cast<size_t>(a) * src_stride + idx[k]];
  }
}

extern "C" int flow_gather_rows(int ncomp, const int* idx, int m,
                                const double* src, int src_stride, double* dst,
                                int dst_stride, void* stream) {
  FLOW_REQUIRE(ncomp >= 1 && m > 0 && idx && src && dst && src_stride > 0 &&
                   dst_stride >= m,
               "gather_rows arguments");
  hipLaunchKernelGGL(gather_rows_kernel, dim3(grid_for(static_cast<long long>(ncomp) * m)),
                     dim3(kBlock), 0, as_stream(stream), ncomp, m, idx, src,
                     src_stride, dst, dst_stride);
  FLOW_CHECK_LAUNCH();
  return FLOW_OK;
}

// y = sum_k a_k x_k, k < nterms <= 6, in one pass
constexpr int kLincombMax = 6;
struct LincombArgs {
  double a[kLincombMax];
  const double* x[kLincombMax];
};
template <int NT>
__global__ void lincomb_kernel(int n, LincombArgs t, double* __restrict__ y) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += gridDim.x * blockDim.x) {
    double v = 0.0;
#pragma unroll
    for (int k = 0; k < NT; ++k) v += t.a[k] * t.x[k][i];
    y[i] = v;
  }
}

// Host arithmetic only (no GPU): the weights of flow_lincomb for an
// extrapolation in time -- see include/flow_hip.h.
extern "C" int flow_extrapolation_weights(int m, const double* dts_host, double dt,
                                          int power, int degree,
                                          double* w_host) {
  FLOW_REQUIRE(m >= 1 && m <= kLincombMax && dts_host && w_host && dt > 0.0,
               "extrapolation weights: 1..6 past steps");
  const int q = (degree <= 0 || degree > m - 1) ? m - 1 : degree;
  const int n = q + 1;
  double x[kLincombMax], t = 0.0;
  for (int i = 0; i < m; ++i) {      // mid points; time 0 = end of the newest
    FLOW_REQUIRE(dts_host[i] > 0.0, "extrapolation weights: step sizes");
    x[i] = t - 0.5 * dts_host[i];
    t -= dts_host[i];
  }
  const double scale = -t;
  for (int i = 0; i < m; ++i) x[i] /= scale;
  const double xs = 0.5 * dt / scale;
  // w = V (V^T V)^-1 e,  V_ik = x_i^k,  e_k = xs^k
  double V[kLincombMax][kLincombMax], N[kLincombMax][kLincombMax + 1];
  for (int i = 0; i < m; ++i) {
    double p = 1.0;
    for (int k = 0; k < n; ++k, p *= x[i]) V[i][k] = p;
  }
  double e = 1.0;
  for (int a = 0; a < n; ++a, e *= xs) {
    for (int b = 0; b < n; ++b) {
      double sum = 0.0;
      for (int i = 0; i < m; ++i) sum += V[i][a] * V[i][b];
      N[a][b] = sum;
    }
    N[a][n] = e;
  }
  for (int c = 0; c < n; ++c) {      // Gauss-Jordan with partial pivoting
    int piv = c;
    for (int r = c + 1; r < n; ++r)
      if (fabs(N[r][c]) > fabs(N[piv][c])) piv = r;
    FLOW_REQUIRE(N[piv][c] != 0.0, "extrapolation weights: singular fit");
    for (int k = 0; k <= n; ++k) {
      const double tmp = N[c][k];
      N[c][k] = N[piv][k];
      N[piv][k] = tmp;
    }
    const double d = N[c][c];
    for (int k = 0; k <= n; ++k) N[c][k] /= d;
    for (int r = 0; r < n; ++r) {
      if (r == c) continue;
      const double f = N[r][c];
      for (int k = 0; k <= n; ++k) N[r][k] -= f * N[c][k];
    }
  }
  for (int i = 0; i < m; ++i) {
    double w = 0.0;
    for (int a = 0; a < n; ++a) w += V[i][a] * N[a][n];
    w_host[i] = w * pow(dt / dts_host[i], power);
  }
  return FLOW_OK;
}

extern "C" int flow_lincomb(int n, int nterms, const double* coef_host,
                            const double* const* x_host, double* y,
                            void* stream) {
  FLOW_REQUIRE(n >= 0 && nterms >= 1 && nterms <= kLincombMax && coef_host &&
                   x_host && y,
               "lincomb arguments (1..6 terms)");
  if (n == 0) return FLOW_OK;
  LincombArgs t = {};
  for (int k = 0; k < nterms; ++k) {
    FLOW_REQUIRE(x_host[k] != nullptr && x_host[k] != y, "lincomb term");
    t.a[k] = coef_host[k];
    t.x[k] = x_host[k];
  }
  const dim3 grid(grid_for(n)), blk(kBlock);
  hipStream_t st = as_stream(stream);
  switch (nterms) {
    case 1: hipLaunchKernelGGL(lincomb_kernel<1>, grid, blk, 0, st, n, t, y); break;
    case 2: hipLaunchKernelGGL(lincomb_kernel<2>, grid, blk, 0, st, n, t, y); break;
    case 3: hipLaunchKernelGGL(lincomb_kernel<3>, grid, blk, 0, st, n, t, y); break;
    case 4: hipLaunchKernelGGL(lincomb_kernel<4>, grid, blk, 0, st, n, t, y); break;
    case 5: hipLaunchKernelGGL(lincomb_kernel<5>, grid, blk, 0, st, n, t, y); break;
    default: hipLaunchKernelGGL(lincomb_kernel<6>, grid, blk, 0, st, n, t, y); break;
  }
  FLOW_CHECK_LAUNCH();
  return FLOW_OK;
}

// ---------------------------------------------------------------------------
// Fingerprints of fields: which trajectory does a call continue?  The start
// vectors of a time loop (flow_amd/navier_stokes/start_vectors.py) belong to
// the trajectory whose last step RETURNED the fields this call is handed; the
// caller copies them (`u0.assign(u1)`, tests/test_karman_vortex_street.py:
// 241-242), so identity is a matter of values.  64-bit sum of the entries' bit
// patterns times odd multipliers of their index, modulo 2^64: integer
// arithmetic, so the order of summation does not matter and equal fields give
// equal fingerprints bit for bit.  Fields beyond 2^22 entries are sampled by
// whole 64-byte lines (every k-th), at most 32 MB read per field.
// ---------------------------------------------------------------------------
constexpr int kFingerprintFields = 2;
struct FingerprintArgs {
  const double* x[kFingerprintFields];
  int n[kFingerprintFields];
  int line_stride[kFingerprintFields];
  int sampled[kFingerprintFields];     // entries visited
};

__global__ __launch_bounds__(kBlock) void fingerprint_kernel(
    FingerprintArgs a, unsigned long long* __restrict__ part) {
  __shared__ unsigned long long wave_part[kBlock / 64];
  const int f = blockIdx.y;
  const double* __restrict__ x = a.x[f];
  const int n = a.n[f], k = a.line_stride[f], m = a.sampled[f];
  unsigned long long h = 0;
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < m;
       e += gridDim.x * blockDim.x) {
    const long long idx = static_cast<long long>(e >> 3) * k * 8 + (e & 7);
    if (idx < n) {
      const unsigned long long bits =
          static_cast<unsigned long long>(__double_as_longlong(x[idx]));
      h += (bits ^ (bits >> 29)) *
           ((2ull * static_cast<unsigned long long>(idx) + 1ull) *
            0x9E3779B97F4A7C15ull);
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) h += __shfl_down(h, off, 64);
  if ((threadIdx.x & 63) == 0) wave_part[threadIdx.x >> 6] = h;
  __syncthreads();
  if (threadIdx.x == 0) {
    h = 0;
    for (int w = 0; w < kBlock / 64; ++w) h += wave_part[w];
    part[static_cast<size_t>(f) * kRedBlocks + blockIdx.x] = h;
  }
}

// one block per field: slots[2f] = low 32 bits, slots[2f+1] = high 32 bits of
// the sum of the partials, as doubles (exact integers: they travel through the
// double-typed mailbox unharmed)
__global__ __launch_bounds__(kBlock) void fingerprint_finish_kernel(
    int nparts, const unsigned long long* __restrict__ part,
    double* __restrict__ slots) {
  __shared__ unsigned long long wave_part[kBlock / 64];
  const int f = blockIdx.x;
  unsigned long long h = 0;
  for (int i = threadIdx.x; i < nparts; i += kBlock)
    h += part[static_cast<size_t>(f) * kRedBlocks + i];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) h += __shfl_down(h, off, 64);
  if ((threadIdx.x & 63) == 0) wave_part[threadIdx.x >> 6] = h;
  __syncthreads();
  if (threadIdx.x == 0) {
    h = 0;
    for (int w = 0; w < kBlock / 64; ++w) h += wave_part[w];
    store_scalar(slots + 2 * f, static_cast<double>(h & 0xffffffffull));
    store_scalar(slots + 2 * f + 1, static_cast<double>(h >> 32));
  }
}

extern "C" int flow_fingerprint(int nfields, const double* const* x_host,
                                const int* n_host, double* work, double* slots,
                                void* stream) {
  FLOW_REQUIRE(nfields >= 1 && nfields <= kFingerprintFields && x_host &&
                   n_host && work && slots,
               "fingerprint arguments (1 or 2 fields)");
  FingerprintArgs a = {};
  int most = 0;
  for (int f = 0; f < nfields; ++f) {
    FLOW_REQUIRE(x_host[f] != nullptr && n_host[f] > 0, "fingerprint field");
    const long long lines = (static_cast<long long>(n_host[f]) + 7) / 8;
    const long long cap = (1ll << 22) / 8;
    const long long k = (lines + cap - 1) / cap;
    a.x[f] = x_host[f];
    a.n[f] = n_host[f];
    a.line_stride[f] = static_cast<int>(k);
    a.sampled[f] = static_cast<int>(((lines + k - 1) / k) * 8);
    if (a.sampled[f] > most) most = a.sampled[f];
  }
  hipStream_t st = as_stream(stream);
  const int g = grid_for(most, kBlock * 4, kRedBlocks);
  unsigned long long* part = reinterpret_cast<unsigned long long*>(work);
  hipLaunchKernelGGL(fingerprint_kernel, dim3(g, nfields), dim3(kBlock), 0, st,
                     a, part);
  hipLaunchKernelGGL(fingerprint_finish_kernel, dim3(nfields), dim3(kBlock), 0,
                     st, g, part, slots);
  FLOW_CHECK_LAUNCH();
  return FLOW_OK;
}

extern "C" int flow_fill(int n, double value, double* y, void* stream) {
  FLOW_REQUIRE(n > 0 && y, "fill arguments");
  return fill(n, value, y, as_stream(stream));
}

extern "C" int flow_vmul(int n, double a, const double* x, const double* y,
                         double* out, void* stream) {
  FLOW_REQUIRE(n > 0 && x && y && out, "vmul arguments");
  hipLaunchKernelGGL(vmul_kernel, dim3(grid_for(n)), dim3(kBlock), 0,
                     as_stream(stream), n, a, x, y, out);
  FLOW_CHECK_LAUNCH();
  return FLOW_OK;
}
