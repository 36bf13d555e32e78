// What the units of the linear-algebra library share among themselves:
// la_kernels.hip (operators, BLAS-1, read-backs), krylov_kernels.hip (CG,
// BiCGStab, GMRES, their preconditioners), shard_kernels.hip (K15) and
// profile_kernels.hip.  What other .hip files use is declared in common.h.
//
// Every kernel is compiled in ONE unit.  A unit that launches a kernel it does
// not own sees a declaration here -- for a template an explicit instantiation
// declaration, with the explicit instantiation definition in the owning unit.
#pragma once
#include "common.h"

namespace flow {

// ---- la_kernels.hip ---------------------------------------------------------
inline int op_size(const flow_operator* A) {
  return A->kind == 0 ? A->n : 2 * A->n;
}

// number of x.Ax partials apply() leaves in dpart
inline int dot_parts(const flow_operator* A) {
  return A->kind == 1 ? 2 * A->nblocks : A->nblocks;
}

// Per-kernel timing of the in-solver SpMV (flow_profile_spmv_begin / _end in
// include/flow_hip.h): while it is on, every launch of the fused-dot SpMV of a
// scalar operator with `rows` rows -- the product with A inside a CG iteration,
// in the cache state the solver leaves -- is bracketed by a pair of HIP events
// on the launch stream.
struct SpmvProfile {
  int rows = 0, cap = 0, used = 0;
  hipEvent_t* ev = nullptr;   // 2 * cap events
};
extern SpmvProfile g_spmv_profile;

// y = A x; with dpart != nullptr also the dot_parts(A) workgroup shares of x.y
// vec_stride: component stride of x and y for the two-component kinds 3 and 4
// (0: A->n); x and y are indexed by global row either way
int apply(const flow_operator* A, const double* x, double* y, hipStream_t st,
          double* dpart = nullptr, const double* stop = nullptr,
          int vec_stride = 0, int out_stride = 0,
          const double* jvp_prm = nullptr);

// block partials of up to three dot products (dot3_kernel)
int dots(int n, int nd, const double* a0, const double* b0, const double* a1,
         const double* b1, const double* a2, const double* b2, double* partial,
         int* nparts, hipStream_t st);

// the calling thread's mailbox: kMailbox doubles of pinned, mapped host memory
constexpr int kMailbox = 64;
// n <= kMailbox doubles of device memory -> the host
int read_values(const double* dev, int n, double* host, hipStream_t st);

__global__ __launch_bounds__(kBlock) void absmax_kernel(
    int n, const double* __restrict__ x, double* __restrict__ partial);
__global__ __launch_bounds__(kBlock) void finish_kernel(
    int nparts, int nd, int is_max, const double* __restrict__ partial,
    double* __restrict__ out);
__global__ void axpby_kernel(int n, double a, const double* __restrict__ x,
                             double b, double* __restrict__ y);
__global__ void vmul_kernel(int n, double a, const double* x, const double* y,
                            double* out, const double* stop = nullptr);
__global__ void residual_kernel(int n, const double* __restrict__ b,
                                const double* __restrict__ q,
                                const double* __restrict__ dinv,
                                double* __restrict__ r, double* __restrict__ z);

// ---- krylov_kernels.hip -----------------------------------------------------
constexpr int kScalarBlock = 1024;   // 16 wavefronts: many partials, one block

template <int UP, bool DOTS>
__global__ __launch_bounds__(kBlock) void mg_level_kernel(
    const int* __restrict__ rowptr, const int* __restrict__ cols,
    const double* __restrict__ vals, const int* __restrict__ rowblocks,
    const double* __restrict__ x, const double* __restrict__ c,
    const double* __restrict__ t, const double* __restrict__ dinv, double omega,
    double* __restrict__ y, double* __restrict__ gpart,
    double* __restrict__ rpart, const double* __restrict__ stop);
template <bool DOTS>
__global__ __launch_bounds__(kBlock) void mg_up2_kernel(
    const int* __restrict__ rowblocks, const int* __restrict__ p_rowptr,
    const int* __restrict__ p_cols, const double* __restrict__ p_vals,
    const int* __restrict__ a_rowptr, const int* __restrict__ a_cols,
    const double* __restrict__ a_vals, const double* __restrict__ xc,
    const double* __restrict__ c, const double* __restrict__ dinv, double omega,
    double* __restrict__ y, double* __restrict__ gpart,
    double* __restrict__ rpart, const double* __restrict__ stop,
    int own_lo = 0, int own_hi = 0x7fffffff);
template <bool DOTS>
__global__ __launch_bounds__(kBlock) void cg_update_kernel(
    int n, const double* __restrict__ S, const double* __restrict__ dinv,
    const double* __restrict__ w, double* __restrict__ z, double* __restrict__ p,
    double* __restrict__ s, double* __restrict__ x, double* __restrict__ r,
    int want_z, double* __restrict__ partial,
    const double* __restrict__ own);

// the instantiations, X(extern template) here, X(template) in the owner
#define FLOW_KRYLOV_INSTANCES(X)                                               \
  X __global__ void mg_level_kernel<0, false>(                                 \
      const int*, const int*, const double*, const int*, const double*,        \
      const double*, const double*, const double*, double, double*, double*,   \
      double*, const double*);                                                 \
  X __global__ void mg_level_kernel<1, false>(                                 \
      const int*, const int*, const double*, const int*, const double*,        \
      const double*, const double*, const double*, double, double*, double*,   \
      double*, const double*);                                                 \
  X __global__ void mg_level_kernel<1, true>(                                  \
      const int*, const int*, const double*, const int*, const double*,        \
      const double*, const double*, const double*, double, double*, double*,   \
      double*, const double*);                                                 \
  X __global__ void mg_up2_kernel<false>(                                      \
      const int*, const int*, const int*, const double*, const int*,           \
      const int*, const double*, const double*, const double*, const double*,  \
      double, double*, double*, double*, const double*, int, int);             \
  X __global__ void mg_up2_kernel<true>(                                       \
      const int*, const int*, const int*, const double*, const int*,           \
      const int*, const double*, const double*, const double*, const double*,  \
      double, double*, double*, double*, const double*, int, int);             \
  X __global__ void cg_update_kernel<false>(                                   \
      int, const double*, const double*, const double*, double*, double*,      \
      double*, double*, double*, int, double*, const double*);                 \
  X __global__ void cg_update_kernel<true>(                                    \
      int, const double*, const double*, const double*, double*, double*,      \
      double*, double*, double*, int, double*, const double*);
FLOW_KRYLOV_INSTANCES(extern template)

int check_mg(const flow_mg* M, int n);
// z = V-cycle(r) from level l0 down (see krylov_kernels.hip)
int vcycle(const flow_mg* M, const double* r0, double* z0, hipStream_t st,
           double* gpart = nullptr, double* rpart = nullptr,
           int* nparts = nullptr, const double* stop = nullptr, int l0 = 0);

// GMRES(m): restart length and the device-resident state of one cycle
// (doubles, behind the partials)
constexpr int kGmresMax = FLOW_GMRES_MAX_RESTART;
constexpr int kGH = 0;                                   // H[col][row]
constexpr int kGNrm = kGH + kGmresMax * (kGmresMax + 1);  // |V_k|
constexpr int kGEta = kGNrm + kGmresMax + 1;              // h_{k+1,k} estimates
constexpr int kGCoef = kGEta + kGmresMax;                 // next vector: c_k
constexpr int kGCw = kGCoef + kGmresMax;                  //   and the w factor
constexpr int kGYc = kGCw + 1;                            // update: y_k / |V_k|
constexpr int kGRot = kGYc + kGmresMax;                   // Givens (cs, sn)[k]
constexpr int kGRhs = kGRot + 2 * kGmresMax;              // rotated beta e1
constexpr int kGJvp = kGRhs + kGmresMax + 1;                // momentum_jvp_params
constexpr int kGState = kGJvp + 3;
static_assert(kGState <= FLOW_GMRES_STATE, "gmres device state");

// out = [accumulate ? out : *cw w] + sum_{k<nv} coef[k] V_k, the coefficients
// in device memory (gmres_combine_dev_kernel)
int gmres_combine_dev(int N, int nv, const double* coef, const double* cw,
                      const double* w, const double* V, double* out,
                      double* nn_partial, bool accumulate, const double* stop,
                      hipStream_t st);
// the restart length and the expected iterations of a GMRES entry point
int check_gmres_args(int restart, int expected_its);

}  // namespace flow

// (the GMRES kernels live outside the namespace)
template <int NV>
__global__ __launch_bounds__(flow::kBlock) void gmres_dots_kernel(
    int n, const double* __restrict__ w, const double* __restrict__ V,
    size_t stride, int with_ww, double* __restrict__ partial,
    double* __restrict__ ww_partial, const double* __restrict__ stop = nullptr);
#define FLOW_GMRES_DOTS_INSTANCES(X)                                           \
  X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8)
#define FLOW_GMRES_DOTS_EXTERN(NV)                                             \
  extern template __global__ void gmres_dots_kernel<NV>(                       \
      int, const double*, const double*, size_t, int, double*, double*,        \
      const double*);
FLOW_GMRES_DOTS_INSTANCES(FLOW_GMRES_DOTS_EXTERN)
#undef FLOW_GMRES_DOTS_EXTERN
// CALL(NV) for a chunk of nv <= 8 basis vectors
#define FLOW_NV_SWITCH(nv, CALL) \
  switch (nv) {                  \
    case 1: CALL(1); break;      \
    case 2: CALL(2); break;      \
    case 3: CALL(3); break;      \
    case 4: CALL(4); break;      \
    case 5: CALL(5); break;      \
    case 6: CALL(6); break;      \
    case 7: CALL(7); break;      \
    default: CALL(8); break;     \
  }
__global__ __launch_bounds__(flow::kBlock) void gmres_step_kernel(
    int nparts, int j, int last, double beta, double target,
    const double* __restrict__ partial, double* __restrict__ G,
    double* __restrict__ S);
