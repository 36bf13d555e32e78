/*
 * flow_hip.h -- C ABI of libflow_hip.so, the MI355X (gfx950) implementation of
 * the Navier-Stokes pressure-correction / heat hot path of nschloe/flow.
 *
 * The reference has no FFI: its boundary is the Python API of
 * flow/navier_stokes/pressure_correction.py (Chorin/IPCS/Rotational.step) and
 * flow/heat.py (Heat).  Every numerical operation the reference delegates to
 * FFC-generated tabulate_tensor + DOLFIN Assembler + PETSc is exported here as
 * a plain-C entry point; each declaration cites the reference lines whose work
 * it replaces (paths relative to the reference root).  The Python host code in
 * flow_amd/ binds these with ctypes.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (HBM) unless the name ends in _host;
 *     the library never allocates or frees device memory and keeps no state
 *     (one exception: a 64-byte host-coherent mailbox per host thread, through
 *     which a kernel of the stream hands scalar results to the host);
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); all
 *     work is enqueued on it; only the *_solve entry points and the *_host
 *     readbacks synchronise it;
 *   - fp64 values, int32 indices; vector fields are component-blocked
 *     (dof (a, i) -> a*n + i);
 *   - per-cell arrays are SoA with the cell index fastest ([k][cell]);
 *   - return codes: 0 ok, 1 not converged, 2 invalid argument, 3 HIP error;
 *     flow_last_error() returns the message of the last failure on the
 *     calling thread.
 */
#ifndef FLOW_HIP_H
#define FLOW_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FLOW_OK 0
#define FLOW_NOT_CONVERGED 1
#define FLOW_INVALID 2
#define FLOW_HIP_ERROR 3

/* CSR-stream tiling of the SpMV kernels (row blocks are built on the host): at
 * most FLOW_SPMV_ROWS_PER_BLOCK rows and flow_spmv_tile_nnz(kind) nonzeros per
 * block -- FLOW_SPMV_NNZ_PER_BLOCK for the kinds that park two products per
 * nonzero in LDS (2 and 4), as many or twice as many for the others (a build
 * constant of the library: ask). */
#define FLOW_SPMV_ROWS_PER_BLOCK 256
#define FLOW_SPMV_NNZ_PER_BLOCK 1022
int flow_spmv_tile_nnz(int kind);

const char* flow_last_error(void);
int flow_abi_version(void);
/* Kernel launches the library has issued so far in this process (all entry
 * points, all streams): differences over a window give launches per step. */
int flow_launch_count(unsigned long long* count_host);
/* Iteration bodies as HIP graphs (flow_amd/csrc/graph_replay.hip) -- OFF by
 * default.  The Krylov and defect-correction loops of this library
 * (flow_cg_solve*, flow_gmres_solve, flow_mass_solve*) issue the same chain of
 * launches every iteration; each can be captured once and replayed, with
 * bit-identical results.  Measured on MI355X / ROCm 7.2 the replay is SLOWER
 * than the launches it replaces at every size of the workload (2.61 against
 * 2.38 ms per step on the eighth-size proxy; graph_replay.hip has the table),
 * hence the default.
 * mode 0 (default, FLOW_AMD_GRAPHS unset): never; 1 (FLOW_AMD_GRAPHS=1): always;
 * 2 (FLOW_AMD_GRAPHS=auto): for systems of up to auto_rows rows (< 0: leave;
 * default 1.5e6, FLOW_AMD_GRAPH_ROWS); mode | (sites << 4) with sites != 0
 * also chooses the loops (1 CG, 2 GMRES, 4 mass solver; default all).  A graph
 * is captured the first time a body is seen and kept under a hash of every
 * value that reaches its kernels (the step size of the matrix-free Jacobian
 * travels through device memory instead); a replay counts as ONE launch in
 * flow_launch_count.
 * flow_graph_stats: stats_host[0..7] = graphs kept, captures so far, replays
 * so far, kernel nodes those replays carried, captures by loop (CG, GMRES,
 * mass solver), 0. */
int flow_graph_mode(int mode, long long auto_rows);
int flow_graph_stats(unsigned long long* stats_host);
/* Host copy of the workgroup -> tile mapping the CSR-stream kernels use
 * (XCD-aware, a permutation of [0, nblocks)); for tests. */
int flow_xcd_tile_host(int block, int nblocks);

/* A linear operator over ONE scalar CSR pattern (n rows, nnz entries).
 *   kind 0: scalar              y = A0 x                      (size n)
 *   kind 1: block diagonal      y_a = A_a x_a, a = 0,1        (size 2n)
 *   kind 2: full 2x2 blocks     y_a = sum_c A_{2a+c} x_c      (size 2n)
 *   kind 3: matrix-free         y = J(ui) x, `matfree` points to a
 *           flow_momentum_jvp (below); no pattern, no value planes (size 2n)
 *   kind 4: one plane, both components, Dirichlet rows by mask   (size 2n)
 *           y_a[i] = rowmask[a*n+i] ? (A0 x_a)[i] : x_a[i]
 *           The "identity rows" form of a component-wise Dirichlet-eliminated
 *           operator whose blocks are the same matrix (the vector mass matrix
 *           of the velocity correction, pressure_correction.py:451-464): on
 *           vectors that vanish on the Dirichlet dofs -- every CG direction
 *           when the start vector carries the boundary values -- it IS the
 *           symmetrically eliminated operator, and the matrix is streamed once
 *           for both components (0.76 GB instead of 1.35 GB per product on the
 *           headline workload).
 * Replaces the PETSc AIJ matrices behind `solve`/`assemble`
 * (pressure_correction.py:224-254, 326-339, 419-432, 451-464; heat.py:88,106). */
typedef struct {
  int kind;
  int n;
  int nnz;
  int nblocks;             /* number of CSR-stream row blocks */
  const int* rowptr;       /* n+1 */
  const int* cols;         /* nnz */
  const int* rowblocks;    /* nblocks+1 */
  const double* vals[4];   /* value planes, nnz each; every plane 16-B aligned
                              and readable up to index nnz (the SpMV loads
                              value PAIRS); cols likewise readable at nnz */
  const void* matfree;     /* kind 3 only: const flow_momentum_jvp* */
  const unsigned char* rowmask;   /* kind 4 only: 2n bytes, 0 = Dirichlet row */
} flow_operator;

/* ---- K8: SpMV (PETSc MatMult inside every Krylov solve; heat.py:101) ---- */
int flow_operator_apply(const flow_operator* A, const double* x, double* y,
                        void* stream);
/* dinv[a*n+i] = 1 / A_aa[i,i]  (K10 Jacobi; replaces 'hypre_amg',
 * pressure_correction.py:331,414,456). diag_idx[i] = position of (i,i). */
int flow_operator_diag_inv(const flow_operator* A, const int* diag_idx,
                           double* dinv, void* stream);

/* Per-kernel timer of the roofline kernel in solver context: from
 * _begin on, up to max_launches launches of the fused-dot CSR-stream SpMV of a
 * scalar operator with `rows` rows -- the product with A inside a CG iteration,
 * with whatever the rest of the iteration left in the caches -- are bracketed by
 * HIP events on the launch stream; _end waits for them and returns the summed
 * durations (microseconds) and the number of launches seen.  One profile at a
 * time, not thread safe: a measuring aid for bench.py. */
int flow_profile_spmv_begin(int rows, int max_launches);
int flow_profile_spmv_end(double* total_us, int* launches);
/* What such an event pair reads around a NULL kernel (median of 33, behind a
 * busy stream): the dispatch latency every bracketed launch includes on top of
 * the kernel's execution time -- a profiler's kernel duration does not. */
int flow_profile_event_overhead(double* overhead_us, void* stream);
/* Launches an empty kernel `profile_marker_kernel` with `id` workgroups (1 ..
 * 1024) on the stream: bench.py brackets its timed steps with ids 1 and 2, and
 * profiles/summarize.py cuts a rocprofv3 kernel trace at those launches instead
 * of at guessed offsets. */
int flow_profile_marker(int id, void* stream);
/* dst[0..n) = src[0..n) with a plain 16-byte-per-lane streaming kernel (n even,
 * buffers 16-byte aligned): the measured copy ceiling of the box,
 * 16 n bytes of traffic per launch; and the same for a kernel that only reads
 * (8 n bytes; sink: one double, never written for finite data): what a
 * read-dominated kernel like the SpMV can be held against. */
int flow_profile_stream_copy(size_t n, const double* src, double* dst,
                             void* stream);
int flow_profile_stream_read(size_t n, const double* src, double* sink,
                             void* stream);

/* ---- K9: BLAS-1 (PETSc VecDot/VecAXPY/VecNorm) -------------------------- */
int flow_dot_host(int n, const double* x, const double* y, double* work,
                  double* result_host, void* stream);
/* vals[k] *= d[row(k)] for a scalar CSR plane of n rows: row equilibration
 * before a Krylov solve that stands in for the reference's sparse LU
 * (flow/heat.py:117-121) */
int flow_scale_rows(int n, const int* rowptr, const double* d, double* vals,
                    void* stream);

/* kind 0: l2, 1: linf (norm(vec,'linf'), tests/test_karman_vortex_street.py:268) */
int flow_norm_host(int n, const double* x, int kind, double* work,
                   double* result_host, void* stream);
int flow_axpby(int n, double a, const double* x, double b, double* y,
               void* stream);                       /* y = a x + b y */
int flow_vmul(int n, double a, const double* x, const double* y, double* out,
              void* stream);                        /* out = a x .* y */
int flow_fill(int n, double value, double* y, void* stream);   /* y = value */
/* 64-bit fingerprints of nfields <= 2 device vectors (sum of the entries' bit
 * patterns times odd multipliers of their index, modulo 2^64 -- integer
 * arithmetic: equal values give equal fingerprints bit for bit; beyond 2^22
 * entries every k-th 64-byte line): which trajectory a call continues is a
 * matter of the VALUES of the fields it is handed (callers copy what a step
 * returns: `u0.assign(u1)`, tests/test_karman_vortex_street.py:241-242).
 * Asynchronous: slots (device, 2*nfields doubles) receive the low and the high
 * 32 bits of each fingerprint as exact integers; x_host / n_host are HOST
 * arrays; work: FLOW_REDUCE_WORK doubles.  flow_read_doubles brings n <= 64
 * doubles of device memory to the host in stream order (one synchronisation). */
int flow_fingerprint(int nfields, const double* const* x_host,
                     const int* n_host, double* work, double* slots,
                     void* stream);
int flow_read_doubles(const double* dev, int n, double* host, void* stream);
/* y = sum_k coef_host[k] * x_host[k], k < nterms <= 6, in one pass (coef_host
 * and the pointer list x_host are HOST arrays; y must not be one of the x): the
 * start vectors a time loop extrapolates from its previous increments */
int flow_lincomb(int n, int nterms, const double* coef_host,
                 const double* const* x_host, double* y, void* stream);
/* Its weights for an extrapolation in time (HOST arithmetic, no GPU): for past
 * increments over steps of sizes dts_host[0 .. m) (newest first, m <= 6), what
 * is smooth in time is the rate increment / dt^power at the mid point of its
 * step; a polynomial of `degree` (<= 0 or >= m: m - 1, interpolation) is fitted
 * through the rates by least squares and evaluated at the middle of the new
 * step of size dt:  increment(dt) ~ sum_i w_host[i] * increment_i. */
int flow_extrapolation_weights(int m, const double* dts_host, double dt,
                               int power, int degree, double* w_host);
/* dst[a*dst_stride + k] = src[a*src_stride + idx[k]], k < m, a < ncomp: the
 * vertex values of a P2 field (the linearisation point of the P1 level of
 * flow_pmg) */
int flow_gather_rows(int ncomp, const int* idx, int m, const double* src,
                     int src_stride, double* dst, int dst_stride, void* stream);
#define FLOW_REDUCE_WORK 4096   /* doubles of `work` the reductions need */

/* Two-level additive preconditioner  z = D^-1 r + P Ac^-1 P^T r  for scalar
 * SPD systems (stands in for the reference's 'hypre_amg', pressure_correction.py
 * :331,414-418): Jacobi plus a piecewise-constant aggregate coarse space whose
 * Galerkin operator Ac = P^T A P is inverted once on the host (dense; for the
 * singular Neumann operator the pseudo-inverse).  Aggregates: agg_of[i] in
 * [0,nc) or -1 (Dirichlet dofs); agg_ptr/agg_dofs list the dofs per aggregate. */
typedef struct {
  int n;                   /* fine dofs */
  int nc;                  /* aggregates */
  const int* agg_ptr;      /* nc+1 */
  const int* agg_dofs;     /* fine dofs sorted by aggregate */
  const int* agg_of;       /* n */
  int lda;                 /* row stride of Ainv in floats, multiple of 4, >= nc */
  const float* Ainv;       /* nc rows of lda floats (pad = 0), 16-B aligned: the
                              coarse inverse is only a preconditioner, so it is
                              kept in fp32 (half the HBM bytes of the per-
                              iteration dense product); sums run in fp64 */
} flow_coarse;

/* Smoothed-aggregation multigrid V(1,1)-cycle as a CG preconditioner for scalar
 * SPD systems (the AMG-class stand-in for 'hypre_amg', pressure_correction.py
 * :331,414-418).  The hierarchy is built once per (operator, BC
 * set) on the host (flow_amd/fem/multigrid.py): aggregates of ~3x3 vertices,
 * prolongation P = (I - 4/(3 rho) D^-1 A) P0, Galerkin operators R A P with
 * R = P^T, until the coarsest level is small enough for a dense (pseudo-)
 * inverse.  One application is the textbook cycle (zero start, one damped-
 * Jacobi sweep before and after the coarse correction)
 *   x = w D^-1 r ; r' = R (r - A x) ; [coarse] ; x += P x' ; x += w D^-1 (r - A x)
 * regrouped so that a level costs three launches and ONE product with A:
 *   t = r - Ah r ; r' = R t ; [coarse] ; x = Ps x' + w D^-1 (r + t)
 * with Ah = A w D^-1 (columns scaled; shares A's pattern arrays) and
 * Ps = (I - w D^-1 A) P, both formed at setup -- or, when the hierarchy also
 * carries C = R (I - Ah) (formed at setup like the Galerkin products) and row
 * blocks common to Ps and Ah, TWO launches:
 *   r' = C r ; [coarse] ; x = Ps x' + w D^-1 (2 r - Ah r)
 * (the second kernel does both products of its rows): no intermediate vector,
 * one launch less per level -- what the small levels' cost consists of --, and
 * on the strips of K15 the restriction needs no ghost rows of r at all.
 * All operators are kind-0 flow_operators (Ps, R, C rectangular: `n` = rows).
 * Levels 0 .. nlevels-1; the last one is solved with the dense inverse. */
#define FLOW_MG_MAX_LEVELS 8
typedef struct {
  int nlevels;
  flow_operator Ah[FLOW_MG_MAX_LEVELS];   /* A[l] w D[l]^-1, l < nlevels-1 (level 0 = the system) */
  const double* dinv[FLOW_MG_MAX_LEVELS]; /* 1 / diag A[l] */
  flow_operator Ps[FLOW_MG_MAX_LEVELS];   /* n_l x n_{l+1} */
  flow_operator R[FLOW_MG_MAX_LEVELS];    /* n_{l+1} x n_l, R = P^T */
  double* r[FLOW_MG_MAX_LEVELS];          /* work vectors of level l >= 1 (n_l) */
  double* x[FLOW_MG_MAX_LEVELS];
  double* t[FLOW_MG_MAX_LEVELS];          /* all levels l < nlevels-1 (n_l) */
  int nc, lda;                            /* coarsest level: size, row stride */
  const float* Ainv;                      /* nc rows of lda floats, as flow_coarse */
  double omega;                           /* Jacobi damping w (0.8) */
  /* the two-launch form: used for ALL levels when C[0].rowptr != NULL */
  flow_operator C[FLOW_MG_MAX_LEVELS];    /* n_{l+1} x n_l: R[l] (I - Ah[l]) */
  const int* up_rowblocks[FLOW_MG_MAX_LEVELS];  /* row blocks of level l that hold
                                             <= flow_spmv_tile_nnz(0) nonzeros of
                                             Ps[l] AND of Ah[l] */
  int up_nblocks[FLOW_MG_MAX_LEVELS];
} flow_mg;
/* z = D^-1 r + P Ac^-1 P^T r: one application of the two-level preconditioner
 * (for callers that drive their own Krylov loop: the preconditioned MINRES of
 * flow_amd/stokes.py).  work: 2*coarse->lda doubles, 16-byte aligned. */
int flow_two_level_apply(const flow_coarse* coarse, const double* dinv,
                         const double* r, double* z, double* work,
                         void* stream);

/* z = V-cycle(r) on level 0 (n = its size): one preconditioner application */
int flow_mg_apply(const flow_mg* mg, int n, const double* r, double* z,
                  void* stream);

/* ---- K11: multicolour ILU(0) ----------------------------------------------
 * (replaces the sparse LU of the Newton solve, pressure_correction.py:224-254,
 * and `LUSolver`, heat.py:117-121, as a BiCGStab preconditioner).  The plan is
 * built once per pattern on the host (flow_amd/fem/ilu.py): rows are ordered by
 * colour (independent sets), so factorisation and both triangular sweeps are
 * one launch per colour.  The sweep streams are sliced ELL: inside a colour the
 * rows are sorted by their L / U row lengths and cut into slices of 64 rows (one
 * wavefront); a slice is stored column-major, padded to its longest row (pad:
 * value 0, column 0), so lane i reads entry k of its row at off + 64 k + i --
 * every load coalesced, the row sum stays in registers, no LDS, no barrier.
 * The *_host members are HOST arrays; everything else is device memory.
 * Factor buffer of one block (lu_size doubles, 16-B aligned):
 *   [0, nnz) combined L\U in the permuted CSR | [off_l, +nnz_l) L stream |
 *   [off_u, +nnz_u) U stream | [off_d, +n) inverse pivots. */
#define FLOW_ILU_SLICE 64
typedef struct {
  int n, nnz, ncolors;
  int nnz_l, nnz_u;          /* entries of the sliced streams INCLUDING padding */
  int off_l, off_u, off_d, lu_size;
  int max_row;               /* longest row of the pattern */
  int nslices;               /* slices over all colours (L and U share them) */
  const int* color_ptr_host; /* ncolors+1 (host): row range of every colour */
  const int* slice_ptr_host; /* ncolors+1 (host): slice range of every colour */
  const int* rowptr;         /* n+1, permuted (colour-major) numbering */
  const int* cols;           /* nnz, ascending per row, permuted numbering */
  const int* diag;           /* n: position of the diagonal entry */
  const int* src_pos;        /* nnz: entry -> position in the operator plane */
  const int* old_of_new;     /* n: permuted row -> original dof */
  const int* new_of_old;     /* n: original dof -> permuted row */
  const int* slice_row;      /* nslices: first row of the slice */
  const int* l_slice_off;    /* nslices+1: entry offsets (multiples of 64) */
  const int* l_cols;         /* nnz_l */
  const int* l_pos;          /* nnz_l: position in the combined factor, -1 = pad */
  const int* u_slice_off;
  const int* u_cols;         /* nnz_u */
  const int* u_pos;
} flow_ilu_plan;
typedef struct {
  const flow_ilu_plan* plan;
  int nblocks;               /* 1 (scalar) or 2 (diagonal blocks of a 2-field op) */
  const double* lu;          /* nblocks * lu_size */
  const float* packed;       /* NULL, or (nnz_l + nnz_u) * nblocks floats filled
                                by flow_ilu0_pack: the sweep streams rounded to
                                fp32, blocks interleaved -- half the bytes per
                                application (fp64 arithmetic throughout; a
                                preconditioner only) */
  int single_vector;         /* with packed: the sweep vector is kept in fp32 as
                                well (8 instead of 16 B per gather; the row
                                sums accumulate in fp64).  The application is
                                then not exactly linear: for FLEXIBLE Krylov
                                methods only -- flow_gmres_solve is one (it
                                keeps Z_j = M^-1 V_j and updates x with it) */
  const void* cycle;         /* NULL, or a const flow_tl* (K19 below): wherever a
                                solver applies this preconditioner it runs the
                                two-level cycle that flow_tl describes instead
                                of the bare sweeps (the flow_ilu a flow_tl names
                                as its smoothers must have cycle == NULL) */
} flow_ilu;
/* HOST routine (setup, no GPU needed): first-fit greedy colouring of the graph
 * of a CSR pattern in row order; colour: n ints out, *ncolors <= 63 */
int flow_color_greedy_host(int n, const int* rowptr, const int* cols,
                           int* colour, int* ncolors);
/* HOST routine: `rounds` passes of Culberson's iterated greedy on a proper
 * colouring (colour / *ncolors in and out): the rows are recoloured first-fit
 * class by class -- classes in reverse order on even passes, largest first on
 * odd ones, rows of a class in row order --, which can never need more colours
 * and usually needs fewer (P2 triangulations: 9 -> 7): every colour less is
 * two dependent launches less per ILU(0) application (K11). */
int flow_color_iterate_host(int n, const int* rowptr, const int* cols,
                            int* colour, int* ncolors, int rounds);
/* factor nblocks (1|2) value planes over the plan's pattern into lu
 * (nblocks * lu_size); the blocks share one pass over the index structure */
int flow_ilu0_factor(const flow_ilu_plan* plan, int nblocks,
                     const double* avals0, const double* avals1, double* lu,
                     void* stream);
/* fill `packed` (16-byte aligned) from the factors in ilu->lu; ilu->packed may
 * point at it from then on.  Call again after every flow_ilu0_factor. */
int flow_ilu0_pack(const flow_ilu* ilu, float* packed, void* stream);
/* z = blockdiag(LU)^-1 r in the ORIGINAL numbering; r, z, work: nblocks*n */
int flow_ilu0_solve(const flow_ilu* ilu, const double* r, double* z,
                    double* work, void* stream);

/* ---- K17: p-multigrid / Chebyshev preconditioner ---------------------------
 * (a second stand-in for the sparse LU of the Newton solve,
 * pressure_correction.py:224-254, as the right preconditioner of
 * flow_gmres_solve).  Two levels on the SAME mesh, both made of CSR-stream
 * products only (no dependent sweeps):
 *   fine    the two diagonal blocks of the assembled Jacobian J = dF1/dui over
 *           the scalar P2 pattern, smoothed with `pre` / `post` steps of the
 *           Chebyshev iteration for D^-1 A on [lam_min, lam_max];
 *   coarse  the P1 discretisation of the same linearised operator (P1 is a
 *           subspace of P2: a vertex dof copies its vertex, an edge dof
 *           averages its two end points), packed the same way;
 *           `coarse_steps` Chebyshev steps from a zero start.
 * One application z = M^-1 r:
 *   x = cheb_pre(r) ; rc = P^T (r - A x) ; xc = cheb_coarse(rc) ;
 *   x += P xc ; x += cheb_post(r - A x).
 * The matrices are stored row-scaled (D^-1 A, entries of size <= ~1) in fp16,
 * the two blocks interleaved: vals = nnz half2 (J00, J11)/diag per nonzero -- 8 B
 * per nonzero with the index; a smoother needs no more (same GMRES counts as
 * with fp64 entries).  Vectors inside are fp32, both components interleaved
 * (float2 per dof): the application is not exactly linear in r -- for FLEXIBLE
 * Krylov methods only (flow_gmres_solve is one).  Rows of Dirichlet dofs are
 * identity rows of J: z = r there (bc_fine); the coarse residual is zeroed on
 * the Dirichlet rows of the coarse operator (bc_coarse), whose rows are
 * identity rows too.
 * Level arrays: CSR-stream row blocks of at most FLOW_SPMV_ROWS_PER_BLOCK rows
 * and FLOW_PMG_NNZ_PER_BLOCK nonzeros (a lane loads nonzeros in QUADS, 16-byte
 * loads: the tile base is aligned down to a multiple of four); cols and
 * vals 16-byte aligned and readable three entries past nnz. */
#define FLOW_PMG_NNZ_PER_BLOCK 2044
typedef struct {
  int n, nnz, nblocks;
  const int* rowptr;       /* n+1 */
  const int* cols;         /* nnz */
  const int* rowblocks;    /* nblocks+1: CSR-stream row blocks */
  const void* vals;        /* nnz half2 (filled by flow_pmg_pack) */
  const float* diag;       /* n float2: diagonal of the two blocks */
  const float* dinv;       /* n float2: 1 / diagonal */
  double lam_min, lam_max; /* Chebyshev interval for D^-1 A (flow_pmg_lambda_max
                              gives the upper end) */
  /* optional: the column indices as 16-bit offsets from the lowest column of
   * each row block (6 B per nonzero instead of 8; nnz ushorts, 16-byte aligned,
   * readable three past nnz); used instead of cols when not NULL.  Needs every
   * block's columns to span < 65536 (flow_pmg_cols16 reports otherwise). */
  const void* cols16;
  const int* cbase;        /* nblocks */
  /* optional: ONE plane for both components -- the mean of the two blocks
   * (they differ by the reaction term of the Newton linearisation, of the size
   * of the off-diagonal blocks the cycle drops; the mean is the Oseen operator)
   * -- as a 32-bit word per nonzero: fp16 value | 16-bit column offset from
   * cbase (4 B per nonzero; nnz words, 16-byte aligned, readable three past
   * nnz; filled by flow_pmg_pack1).  Used instead of vals / cols16 when not
   * NULL; idrows (2 n, component-blocked) flags the identity rows of each
   * component, which the plane cannot carry. */
  const void* packed;
  const unsigned char* idrows;
} flow_pmg_level;
typedef struct {
  flow_pmg_level fine, coarse;
  int pre, post, coarse_steps;     /* Chebyshev steps: pre, post 1..3, coarse >= 1 */
  const int* ends;                 /* fine.n int2: coarse rows of a fine dof */
  const int* rptr;                 /* coarse.n+1: restriction lists ... */
  const int* rsrc;                 /* ... of fine dofs; the FIRST entry of a list
                                      is the vertex's own dof (weight 1), the
                                      others are edge dofs (weight 1/2) */
  const unsigned char* bc_fine;    /* 2*fine.n bytes (component-blocked), NULL: none */
  const unsigned char* bc_coarse;  /* 2*coarse.n bytes, NULL: none */
  float* work;                     /* 12*fine.n + 8*coarse.n + 2 floats, 16-B
                                      aligned; the LAST float2 must be zero and
                                      is never written (dummy coarse row) */
  int scalar;                      /* != 0: a SCALAR operator of size fine.n (the
                                      heat system, flow/heat.py:103-122): both
                                      planes of the levels hold the same matrix,
                                      r and z have fine.n entries, the masks are
                                      duplicated; 0: the two velocity blocks */
} flow_pmg;
/* vals[k] = half2((a00, a11)[k] / their diagonal entries of row(k)), 0 where
 * keep[k] == 0 (keep = NULL: everything is kept);
 * diag[i] = (a00, a11)[diag_idx[i]], dinv[i] = 1 / diag[i].
 * K15, block Jacobi on a strip: the level is a rank's DIAGONAL BLOCK in local
 * numbering -- rowptr / diag_idx / a00 / a11 shifted to the block's first
 * nonzero, cols in local numbering with the couplings that leave the block
 * pointing at their own row and marked keep = 0; `ends` of a dof whose partner
 * vertex lies outside names the dummy coarse row coarse.n (work carries a zero
 * there), the restriction lists hold the block's own dofs only. */
int flow_pmg_pack(int n, int nnz, const int* rowptr, const int* diag_idx,
                  const double* a00, const double* a11,
                  const unsigned char* keep, void* vals, float* diag,
                  float* dinv, void* stream);
/* The one-plane stream of a level (flow_pmg_level.packed) from the same two
 * blocks: idrows[a n + i] = 1 where row i of block a has no off-diagonal entry
 * (a Dirichlet dof of component a: found here, the caller passes no mask);
 * entry (i, j) = mean of a00 / a11 over the components in which neither row i
 * nor column j is such a dof, divided by the mean diagonal over the free
 * components of row i, rounded to fp16 and packed with the column offset from
 * cbase[tile] (flow_pmg_cols16 of the same row blocks, no overflow); diag /
 * dinv as flow_pmg_pack's with the free components' entries replaced by the
 * mean.  keep as in flow_pmg_pack. */
int flow_pmg_pack1(int n, int nnz, int nblocks, const int* rowblocks,
                   const int* rowptr, const int* cols, const int* diag_idx,
                   const double* a00, const double* a11,
                   const unsigned char* keep, const int* cbase,
                   unsigned char* idrows, void* packed, float* diag,
                   float* dinv, void* stream);
/* cols16 / cbase of a level's pattern; *overflow_dev (zeroed by the caller) is
 * set when an offset does not fit in 16 bits */
int flow_pmg_cols16(int nblocks, const int* rowblocks, const int* rowptr,
                    const int* cols, int* cbase, void* cols16,
                    int* overflow_dev, void* stream);
/* spectral radius of D^-1 A of a level by `iterations` (>= 2) steps of the
 * power method (normalised on the device: one read-back, at the end).  work:
 * 6*n floats, dwork: FLOW_REDUCE_WORK doubles.  start (optional, 2*n floats,
 * zero before the first call): the iterate the previous call left there is
 * where this one starts (a rebuild of the same level a few time steps later
 * needs a few iterations, not 32) and leaves its own. */
int flow_pmg_lambda_max(const flow_pmg_level* level, int iterations, float* work,
                        double* dwork, float* start, double* result_host,
                        void* stream);
/* z = M^-1 r (r, z: 2*fine.n doubles, component-blocked) */
int flow_pmg_apply(const flow_pmg* pmg, const double* r, double* z, void* stream);

/* HOST routine (setup, no GPU needed): ALGEBRAIC aggregation of the rows of a
 * scalar CSR matrix for the smoothed-aggregation hierarchy (flow_mg below;
 * `hypre_amg` of pressure_correction.py:331, 414 needs no coordinates either).
 * j is strongly coupled to i when |a_ij| >= theta sqrt(|a_ii a_jj|), i != j.
 * Three passes in row order (Vanek, Mandel, Brezina 1996): (1) a free row none
 * of whose strong neighbours is aggregated yet founds an aggregate with all of
 * them; (2) every remaining row joins the aggregate of its strongest coupled
 * aggregated neighbour; (3) what is left forms aggregates with its own
 * unaggregated strong neighbours (isolated rows: singletons).  free[i] == 0
 * (Dirichlet rows; NULL: all free): agg[i] = -1.  agg: n ints out,
 * *naggregates the count.  Deterministic. */
int flow_aggregate_host(int n, const int* rowptr, const int* cols,
                        const double* vals, double theta,
                        const unsigned char* free_rows, int* agg,
                        int* naggregates);

/* ---- K19: two-level cycle with ILU(0) smoothing ----------------------------
 * (the stand-in for the sparse LU of the Newton solve, pressure_correction.py:
 * 224-254, and of the heat solve, heat.py:117-121, WHERE THE CHEBYSHEV CYCLE OF
 * K17 IS REJECTED by its acceptance test: cell Peclet numbers beyond ~3 at
 * CFL-sized steps put the spectrum of D^-1 A off the real axis; a polynomial
 * smoother amplifies there, a multicolour ILU(0) sweep does not.)  The levels are
 * those of K17 -- the diagonal block(s) of the assembled operator on the P2
 * pattern and the P1 discretisation of the same operator on the same mesh, the
 * same transfer tables -- with one ILU(0) application (K11) as the smoother on
 * the fine level and `coarse_sweeps` of them as the treatment of the P1 level.
 * One application z = M^-1 r (all vectors fp64, component-blocked):
 *   x = pre ? ILU_f^-1 r : 0 ;  t = r - A_f x ;  rc = P^T (rscale .* t) ;
 *   xc = ILU_c^-1 rc ; (coarse_sweeps - 1) x [ xc += ILU_c^-1 (rc - A_c xc) ] ;
 *   x += P xc ;  post: x += ILU_f^-1 (r - A_f x) ;  z = x.
 * Measured (tools/smoother_lab.py, flexible GMRES applications to 1e-8):
 * structured channel at cell Peclet 3.5 27 -> 13, graded unstructured channel
 * 48 -> 17, heat system at cell CFL 6 / 14 / 40: 56 / 80 / 146 -> 19 / 23 / 35
 * (two coarse sweeps: 14 / 17 / 28).
 * Dirichlet dofs: identity rows of both operators (ILU: z = r there); the
 * prolongation leaves them alone (bc_fine), the restricted residual is zeroed
 * on those of the P1 level (bc_coarse).  rscale (optional): the residual is
 * multiplied row by row before it is restricted -- the heat solve works on the
 * ROW-SCALED system (ILU(0) is invariant under a row scaling, the rediscretised
 * P1 level is not).  Reached through flow_ilu.cycle by every solver that takes
 * a flow_ilu. */
typedef struct {
  const flow_ilu* fine;          /* ILU(0) of the fine diagonal block(s); cycle == NULL */
  const flow_ilu* coarse;        /* ILU(0) of the P1 level; same nblocks; cycle == NULL */
  const flow_operator* fine_op;  /* A_f, size nblocks * fine->plan->n (kind 0, 1, 2 or 3) */
  const flow_operator* coarse_op;/* A_c (needed for coarse_sweeps > 1) */
  int pre, post;                 /* 0 | 1, not both 0 */
  int coarse_sweeps;             /* 1 .. 8 */
  const int* ends;               /* fine n int2: the coarse rows of a fine dof  } as in */
  const int* rptr;               /* coarse n + 1: restriction lists ...         } flow_pmg */
  const int* rsrc;               /* ... of fine dofs, the vertex's own dof first */
  const unsigned char* bc_fine;  /* nblocks * n bytes or NULL */
  const unsigned char* bc_coarse;/* nblocks * n1 bytes or NULL */
  const double* rscale;          /* nblocks * n or NULL */
  double* work;                  /* nblocks * (4 n + 5 n1) doubles, 16-B aligned */
} flow_tl;
/* z = M^-1 r (r, z: nblocks * n doubles, r != z) */
int flow_tl_apply(const flow_tl* tl, const double* r, double* z, void* stream);

/* ---- K18: mass-matrix solves by mixed-precision defect correction ---------
 * The velocity correction (pressure_correction.py:436-465: `solve(a3 == L3,
 * u1, bcs)`, CG + hypre_amg, relative tolerance tol) and the callers' L2
 * projections (tests/test_karman_vortex_street.py:262-267) are solves with a
 * finite-element MASS matrix.  Its Jacobi-scaled spectrum is known a priori on
 * any mesh (Wathen 1987: the extreme eigenvalues of D^-1 M lie between those
 * of the scaled element matrices -- P1 triangles [1/2, 2], P2 triangles
 * [0.3924, 2.0598]), so a fixed Chebyshev polynomial of D^-1 M is an
 * approximate inverse B with a KNOWN contraction |I - B M| <= eps_k =
 * 2 s^k / (1 + s^2k), s = 0.39 for P2 (k = 6 steps: 7e-3).  The solve is the
 * defect correction
 *     r = b - M x  (fp64, the CSR-stream SpMV of the operator, with the
 *                   residual scaled by D^-1 and rounded to fp32 in its epilogue)
 *     z = B r      (k Chebyshev steps = k - 1 products with a copy of D^-1 M
 *                   rounded to fp16 -- ONE value plane, 6 B per nonzero with
 *                   the index, also when it serves both velocity components --,
 *                   vectors fp32, components interleaved)
 *     x += z       (fp64, in the last product's epilogue)
 * No dot product steers the iteration; one launch per product.  Stopping test:
 * z_k = B r_k IS the preconditioned residual of PETSc's KSPCG test with a
 * preconditioner as strong as the reference's AMG (B ~ M^-1), and B b ~ x:
 *     contraction * |z_k| <= max(rtol |x_k + z_k|, atol)
 * -- since B r_{k+1} = (I - B M) z_k, the iterate x_{k+1} = x_k + z_k then
 * satisfies |B r_{k+1}| <= rtol |B b| (contraction = the bound on |I - B M|
 * the caller vouches for; 1: test |z_k| itself, one more iteration).  Decided
 * on the device like the Krylov drivers below (sticky flag, exact count).
 * A: kind 0 (scalar) or kind 4 (one plane for both components, identity rows
 * by mask; x should carry b on those rows on entry, else it converges there
 * like everywhere).  dinv: op-size doubles (1 on masked rows).
 * vals16: nnz halfs (D^-1 M)_ij (flow_mass_pack), 16-byte aligned, readable
 * three entries past nnz like A->cols (quads of nonzeros per lane);
 * rowblocks16: CSR-stream row blocks of <= FLOW_PMG_NNZ_PER_BLOCK nonzeros.
 * work16: 5 * ncomp * n floats, 16-byte aligned. */
typedef struct {
  const flow_operator* A;
  const double* dinv;
  int nblocks16;
  const int* rowblocks16;
  const void* vals16;
  double lam_min, lam_max;     /* Chebyshev interval of D^-1 M */
  int steps;                   /* Chebyshev steps per defect correction, 3..16 */
  double contraction;          /* bound on |I - B M| in (0, 1] */
  float* work16;
  /* the PACKED stream (used instead of vals16 + A->cols when not NULL): one
   * 32-bit word per nonzero, fp16 value | (column - cbase16[tile]) << 16 --
   * 4 B per nonzero and one 16-byte load per quad of nonzeros; nnz words,
   * 16-byte aligned, readable three past nnz.  Needs every tile's columns to
   * span < 65536 (flow_mass_pack16 reports otherwise). */
  const void* packed16;
  const int* cbase16;          /* nblocks16: lowest column of each tile */
  int work16_rows;             /* rows the fp32 work vectors cover (0: A->n); K15:
                                  the rank's window, flow_shard_mass_solve */
} flow_mass;
/* vals16[k] = half(vals[k] / vals[diag_idx[row(k)]]) */
int flow_mass_pack(int n, const int* rowptr, const int* diag_idx,
                   const double* vals, void* vals16, void* stream);
/* the packed stream of the same matrix over the row blocks rowblocks16;
 * *overflow_dev (an int the caller zeroes) is set to 1 when a column offset
 * does not fit in 16 bits: keep the plain stream then */
int flow_mass_pack16(int n, int nblocks16, const int* rowblocks16,
                     const int* rowptr, const int* cols, const int* diag_idx,
                     const double* vals, int* cbase16, void* packed16,
                     int* overflow_dev, void* stream);
/* x holds the initial guess.  maxit / *iters_host count defect corrections;
 * first_check: as flow_cg_solve (then one at a time).  *resid_host = |z| of
 * the last correction.  work: FLOW_REDUCE_WORK + 2 * nblocks16 doubles. */
int flow_mass_solve(const flow_mass* M, const double* b, double* x, double rtol,
                    double atol, int maxit, int first_check, double* work,
                    size_t work_len, int* iters_host, double* resid_host,
                    void* stream);

/* The same for a solve whose start xbase is close, in INCREMENT form:
 * M (x - xbase) = g with the defect g = b - M xbase GIVEN by the caller -- the
 * velocity correction's is -dt/rho (grad phi, v), assembled without the
 * (ui, v) term (flow_assemble_correction_rhs, flag bit 1) -- and the increment
 * iterated from zero in a vector of its own: the first correction needs no
 * product with M, and fp64 only has to resolve the increment.  delta0 (or
 * NULL): a start vector for the increment (a time loop's previous increments,
 * extrapolated; the first defect is then g - M delta0).  The stopping
 * test is the one above with |x| = |xbase + increment|.  x = xbase + increment
 * on return (x may be xbase; the rows A masks as identity rows need g = 0).
 * work: FLOW_REDUCE_WORK + 2 * nblocks16 + 1 + op-size doubles. */
int flow_mass_solve_increment(const flow_mass* M, const double* g,
                              const double* xbase, const double* delta0,
                              double* x, double rtol,
                              double atol, int maxit, int first_check,
                              double* work, size_t work_len, int* iters_host,
                              double* resid_host, void* stream);

/* The increment solve of a time loop's velocity correction AROUND THE CALLER'S
 * VECTORS (kind 4 only).  Computes, bit for bit, what
 *     start = ui;  start[bc_dofs] = bc values;  delta0[bc_dofs] = 0;
 *     flow_mass_solve_increment(M, g, start, delta0, x_out, ...);
 *     inc_out = x_out - ui
 * computes, with these passes gone: `start` is never formed (the rows read ui,
 * the identity rows xbc: the boundary values scattered into a vector of op
 * size, read on those rows only); delta0 is read where it lies by the first
 * correction (zeroed on the rows bc_dofs IN PLACE first: nbc entries, which
 * must be the rows A masks); the last Chebyshev step of every correction
 * stores x_out = start + increment and inc_out = x_out - ui (or NULL) next to
 * the increment, so nothing runs behind the solve, however it ends.
 * delta0 NULL: the increment starts from zero.  x_out, inc_out: vectors of
 * their own.  Errors, counts, *resid_host and work as
 * flow_mass_solve_increment. */
int flow_mass_correct(const flow_mass* M, const double* g, const double* ui,
                      const double* xbc, double* delta0, int nbc,
                      const int* bc_dofs, double* x_out, double* inc_out,
                      double rtol, double atol, int maxit, int first_check,
                      double* work, size_t work_len, int* iters_host,
                      double* resid_host, void* stream);

/* ---- K12: Krylov drivers -------------------------------------------------
 * Device-resident loops.  Convergence is decided ON THE DEVICE: the kernel
 * that computes the solver scalars compares the residual norm with the target
 * and freezes the solution at the first iterate that passes (everything
 * enqueued behind it returns at once), so *iters_host is the exact count and
 * the solution never moves past the accepted iterate, however late the host
 * looks: it reads the state every check_every iterations -- the first time
 * after first_check iterations when that is > 0 (a time loop knows how many the
 * previous step needed; every read-back drains the stream).
 * Stopping test: CG tests the PRECONDITIONED residual like PETSc's KSPCG (the
 * default the reference's `solve` runs with, pressure_correction.py:326-339,
 * 419-432, 451-464): ||B r||_2 <= max(rtol*||B b||_2, atol), B = the
 * preconditioner (Jacobi, two-level, V-cycle; identity without one) -- with
 * Dirichlet rows carrying boundary VALUES in b next to O(h^2) interior
 * entries, the unpreconditioned norm would let the interior equations off at
 * rtol*|g|/h^2.  *resid_host is that norm.  BiCGStab and GMRES are right-
 * preconditioned: ||r||_2 <= max(rtol*||b||_2, atol).  Return
 * FLOW_NOT_CONVERGED after maxit iterations (dolfin raises RuntimeError:
 * 'error_on_nonconvergence', pressure_correction.py:337,424,462).
 * dinv may be NULL (no preconditioner).  x holds the initial guess.
 * coarse may be NULL (Jacobi only); mg != NULL selects the multigrid V-cycle
 * instead (coarse must then be NULL); ilu may be NULL (Jacobi), else it replaces
 * dinv as the (right) preconditioner of BiCGStab.
 * work (16-byte aligned): FLOW_REDUCE_WORK + 5*N + B + 2 [+ 2*coarse->lda]
 * [+ 2*mg->Ps[0].nblocks] doubles (cg; B = nblocks, twice that for kind 1: the
 * SpMV leaves its z.Az partials there, the V-cycle's last kernel its r.z and
 * z.z partials), FLOW_REDUCE_WORK + 7*N [+ n] (bicgstab); N = operator size. */
int flow_cg_solve(const flow_operator* A, const double* dinv,
                  const flow_coarse* coarse, const flow_mg* mg,
                  const double* b, double* x,
                  double rtol, double atol, int maxit, int check_every,
                  int first_check, double* work, size_t work_len,
                  int* iters_host, double* resid_host, void* stream);
/* flow_cg_solve from a GUARDED start vector (the start vectors a time loop
 * extrapolates from its previous calls, flow_amd/navier_stokes/
 * start_vectors.py; the reference starts every solve from a fresh, zero
 * Function, pressure_correction.py:313).  A start that leaves a larger
 * preconditioned residual than x = 0 would, ||B(b - A x)|| > ||B b|| --
 * decided on the device by the kernel that forms the first iteration's scalars,
 * from numbers it forms anyway; everything enqueued behind the verdict returns
 * at once, x still holds the start -- is dropped for x_fallback (guarded the
 * same way; NULL: none; must not alias x) and that for zero.
 * *starts_dropped_host: 0, 1 or 2.  Everything else as flow_cg_solve. */
int flow_cg_solve_guarded(const flow_operator* A, const double* dinv,
                          const flow_coarse* coarse, const flow_mg* mg,
                          const double* b, double* x, const double* x_fallback,
                          double rtol, double atol, int maxit, int check_every,
                          int first_check, double* work, size_t work_len,
                          int* iters_host, double* resid_host,
                          int* starts_dropped_host, void* stream);
int flow_bicgstab_solve(const flow_operator* A, const double* dinv,
                        const flow_ilu* ilu, const double* b, double* x,
                        double rtol, double atol, int maxit, int check_every,
                        int first_check, double* work, size_t work_len,
                        int* iters_host, double* resid_host, void* stream);
/* GMRES(restart), right-preconditioned with the p-multigrid / Chebyshev cycle
 * (pmg != NULL), ILU(0) (ilu != NULL), Jacobi (dinv != NULL) or nothing -- at
 * most one of pmg / ilu: the Newton systems of the tentative velocity
 * (pressure_correction.py:224-254) -- one operator + preconditioner application
 * per iteration, ~15 % fewer of them than BiCGStab needs there.  Classical
 * Gram-Schmidt with one reduction per iteration; the Hessenberg matrix, the
 * small least-squares problem and the stopping test live on the device (one
 * workgroup behind the dot products), so the Arnoldi steps are enqueued
 * without the host in between: expected_its of them (what the caller expects
 * the solve to need -- the count of the previous solve in a time loop; 0:
 * unknown) before the host looks for the first time, then one at a time.  The
 * accepted iterate does not depend on it: everything enqueued behind it returns
 * at once.  A cycle stops on the least-squares residual estimate.  verify != 0:
 * the iterate is then checked with the true residual b - A x (one more
 * operator application and read-back, not counted): accepted within a factor
 * 10 of the target, with the TRUE norm in *resid_host, continued otherwise --
 * for solves nothing else checks (flow/heat.py:117-121); verify = 0: the
 * estimate is trusted (*resid_host = the estimate) -- the Newton systems, whose
 * outer iteration recomputes the nonlinear residual anyway.  `iters_host` =
 * operator applications of the Arnoldi steps.
 * x_is_zero != 0: the caller guarantees x = 0 on entry (Newton increments), the
 * initial residual is then b without an operator application.
 * work: FLOW_REDUCE_WORK + (2*restart + 2)*N + FLOW_GMRES_PARTIALS +
 * FLOW_GMRES_STATE doubles (the preconditioned basis vectors are kept: no extra
 * preconditioner application for the solution update). */
#define FLOW_GMRES_MAX_RESTART 30
#define FLOW_GMRES_PARTIALS ((FLOW_GMRES_MAX_RESTART + 2) * 1024)
#define FLOW_GMRES_STATE 1280
int flow_gmres_solve(const flow_operator* A, const double* dinv,
                     const flow_ilu* ilu, const flow_pmg* pmg, const double* b,
                     double* x,
                     double rtol, double atol, int maxit, int restart,
                     int x_is_zero, int expected_its, int verify, double* work,
                     size_t work_len, int* iters_host, double* resid_host,
                     void* stream);

/* ---- K15: domain decomposition over the GPUs of one node -------------------
 * (nothing in the reference: DOLFIN/PETSc would do this implicitly under
 * mpirun).  One process per GPU.  The mesh is cut into strips along the channel:
 * with the x-major numbering every scalar space splits into contiguous row
 * blocks, rank g OWNS the rows [r0, r1) and needs, for anything its rows are
 * coupled to (matrix columns, dofs of incident cells), the GHOST rows [e0, r0)
 * and [r1, e1) -- owned by its left and right neighbour.
 *
 * The library needs ONE communication primitive, handed in as a callback:
 *   allreduce(user, count): sum the first `count` doubles of comm->buf over the
 *   ranks, in stream order (kernels enqueued before it have written buf, kernels
 *   enqueued after it see the sums).
 * The host binds it to torch.distributed.all_reduce on RCCL (flow_amd/
 * parallel.py).  Everything travels in that buffer: dot products, the partial
 * coarse residual of the multigrid cycle, and the halos -- every rank writes
 * its boundary rows into its own slots and zeros into all others, so the sum
 * is the concatenation (bitwise the owners' values: x + 0).  One kind of
 * collective, a fixed reduction order, identical results on every rank.
 *
 * Vectors inside the sharded solvers are EXT-COMPACT: ncomp * (e1 - e0)
 * doubles, entry (a, row) at a*(e1-e0) + row - e0.  Kernels that index by
 * global row get the base pointer shifted by -e0 and the component stride
 * e1 - e0; fields handed in by the caller (b, x, dinv, ...) are global-length
 * (stride n), valid on the rank's owned + ghost rows. */
typedef int (*flow_allreduce_fn)(void* user, int count);
/* Halos from neighbour to neighbour instead of through the all-reduce (round
 * 6; optional).  Every rank owns a peer block its two neighbours have mapped
 * with hipIpcOpenMemHandle (xGMI peers on a node; processes sharing one device
 * in a rehearsal): FLOW_PEER_FLAGS 64-bit words, then two landing buffers of
 * land_cap doubles.  One exchange is then a PUSH launch (my send slots of the
 * packed buffer -> the neighbour's landing buffer, then its `arrived` word), the
 * all-reduce of what is really summed (nothing for a pure halo), and a PULL
 * launch (wait for my `arrived` words, landing buffer -> my packed buffer,
 * acknowledge in the neighbour's `consumed` word: it may reuse the buffer two
 * exchanges on).  Sequence numbers count the exchanges of the communicator:
 * every rank issues the same sequence.  Waits are bounded (spin_limit polls):
 * a neighbour that never arrives sets word 4 of the waiting rank's block
 * ((seq << 8) | what it waited for) and the kernel goes on -- the device
 * cannot hang; flow_peer_status reads that word. */
#define FLOW_PEER_FLAGS 16
typedef struct {
  unsigned long long* flags;       /* this rank's block: [arrived L, arrived R,
                                      consumed L, consumed R, error, ...] */
  double* land;                    /* this rank's 2 * land_cap doubles */
  int land_cap;
  int spin_limit;                  /* polls before a wait gives up */
  unsigned long long* nb_flags[2]; /* the neighbours' blocks as mapped HERE ... */
  double* nb_land[2];              /* ... and their landing buffers; NULL: no
                                      neighbour on that side (0 left, 1 right) */
  unsigned long long* seq_host;    /* HOST, 5 words kept by the library: the
                                      counter of this communicator's exchanges,
                                      then per side and landing buffer the
                                      exchange of this rank's last push into it */
} flow_peer;
typedef struct {
  int rank, world;
  double* buf;               /* exchange buffer (device), `capacity` doubles */
  int capacity;
  flow_allreduce_fn allreduce;
  void* user;
  const flow_peer* peer;     /* NULL: halos travel in the all-reduce */
} flow_comm;
/* A peer block of FLOW_PEER_FLAGS words + 2 * land_cap doubles, zeroed, and its
 * 64-byte IPC handle (handle_out); the neighbours map it with flow_peer_open
 * and unmap it with flow_peer_close before the owner frees it. */
int flow_peer_alloc(int land_cap, void** base_out, char* handle_out);
int flow_peer_open(const char* handle, void** base_out);
int flow_peer_close(void* mapped_base);
int flow_peer_free(void* base);
/* the error word of this rank's block (0: every wait so far was served) */
int flow_peer_status(const flow_peer* peer, unsigned long long* error_host,
                     void* stream);

/* The same primitive issued by the library itself: ncclAllReduce on `stream`,
 * on a communicator of its own (flow_amd/csrc/rccl_direct.hip).  The RCCL
 * shared object is dlopen'ed by path (the instance the host already loaded),
 * the 128-byte unique id of rank 0 is distributed by the host.  Set
 * comm->allreduce = flow_rccl_allreduce and comm->user = &binding. */
#define FLOW_RCCL_ID_BYTES 128
typedef struct {
  void* comm;                /* from flow_rccl_comm_create */
  double* buf;               /* = flow_comm.buf */
  void* stream;              /* hipStream_t of the solvers */
} flow_rccl_binding;
int flow_rccl_load(const char* librccl_path);
int flow_rccl_unique_id(char* id_host);                      /* 128 bytes out */
int flow_rccl_comm_create(const char* id_host, int rank, int world,
                          void** comm_out);                  /* collective */
int flow_rccl_comm_destroy(void* comm);
int flow_rccl_allreduce(void* user, int count);              /* flow_allreduce_fn */

/* the rows of one scalar space as rank `comm->rank` sees them; index 0 = left
 * neighbour, 1 = right neighbour, len 0 = none */
typedef struct {
  int n;                     /* global rows */
  int r0, r1;                /* owned */
  int e0, e1;                /* owned + ghost: e0 <= r0 < r1 <= e1 */
  int nhalo;                 /* halo slots of ONE component, all ranks together */
  int send_row[2], send_len[2], send_slot[2];  /* x[row..+len) -> slots */
  int recv_row[2], recv_len[2], recv_slot[2];  /* slots -> x[row..+len) */
} flow_rows;

/* make the ghost rows of x current (ncomp components, x[a*stride + row] with
 * GLOBAL row: a global-length field has stride n; for an ext-compact vector v
 * pass x = v - e0, stride = e1 - e0).  One collective. */
int flow_shard_halo(const flow_comm* comm, const flow_rows* rows, int ncomp,
                    double* x, int stride, void* stream);
/* kind 0: sum over the owned rows of x_a[row] * y_a[row], summed over the
 * ranks; kind 1: max |x| over the owned rows and the ranks (y unused).
 * work: FLOW_REDUCE_WORK doubles.  One collective + one read-back. */
int flow_shard_reduce_host(const flow_comm* comm, const flow_rows* rows,
                           int ncomp, const double* x, const double* y,
                           int stride, int kind, double* work,
                           double* result_host, void* stream);

/* CG + Jacobi on the strips: the mass-matrix solves of the velocity correction
 * (operator kind 4: both components, pressure_correction.py:451-464) and of the
 * callers' step-size projection (kind 0).  A carries the CSR-stream row blocks
 * of the OWNED rows only; b, x, dinv are global-length fields (b valid on the
 * owned rows, x on owned rows -- its ghosts are made current on entry and on
 * exit).  Chronopoulos-Gear recurrences on the owned AND ghost rows (pointwise
 * given w = A z there), so ONE collective per iteration carries the three dot
 * products and the halo of w; stopping test, device-side convergence flag and
 * the meaning of first_check / check_every as flow_cg_solve.  Every rank runs
 * the same number of iterations (the sums are bitwise identical).
 * start_rejected_host != NULL: the start vector is guarded as in
 * flow_cg_solve_guarded -- ||B(b - A x)|| > ||B b|| (sums over all ranks: the
 * same verdict everywhere) leaves x untouched, sets *start_rejected_host = 1
 * and returns FLOW_OK: the caller swaps in its fallback and calls again.
 * work (16-B aligned): FLOW_REDUCE_WORK + 10 * ncomp * (e1 - e0) + A->nblocks
 * + 2 doubles, ncomp = 1 (kind 0) or 2 (kind 4). */
int flow_shard_cg_solve(const flow_comm* comm, const flow_rows* rows,
                        const flow_operator* A, const double* dinv,
                        const double* b, double* x, double rtol, double atol,
                        int maxit, int check_every, int first_check,
                        double* work, size_t work_len, int* iters_host,
                        double* resid_host, int* start_rejected_host,
                        void* stream);

/* The pressure solve on the strips: CG preconditioned with the SAME smoothed-
 * aggregation V(1,1) cycle as flow_cg_solve (same iteration counts).  The
 * finest level is row-sharded: Ah0 / Ps0 are mg->Ah[0] / mg->Ps[0] with the row
 * blocks of the owned rows, Rg is mg->R[0] restricted to the owned COLUMNS
 * (column index minus r0; all coarse rows): every rank restricts its own part
 * of the fine residual, the partial coarse residuals are summed by the
 * collective, and the levels below (a tenth of the rows, latency-bound on one
 * GPU already) run replicated on every rank.  Three collectives per iteration:
 * [dots + halo of w], [coarse residual], [halo of z] -- or, when the hierarchy
 * carries the two-launch form (mg->C) and Cg / up_rowblocks0 are given, TWO:
 * the coarse residual rc = C r is then carried by the recurrences of CG itself,
 *     rc_s = rc_w + beta rc_s ;  rc_r -= alpha rc_s ,   rc_w = C w = sum over
 *     the ranks of Cg w_owned,
 * whose only collective part, rc_w, rides with the dots and the halo of w (C is
 * restricted by COLUMNS: a rank needs no ghost rows for its share).  Every
 * eighth iteration rc_r and rc_s are recomputed from r and s themselves (one
 * more collective then): carried by recurrence alone they drift away from the
 * rank-local vectors and CG stagnates short of a tight target.
 * work: FLOW_REDUCE_WORK + 11 * (e1 - e0) + A->nblocks +
 * 2 * max(Ps0.nblocks, up_nblocks0) + 2 [+ 3 * Cg.n]. */
typedef struct {
  const flow_mg* mg;
  flow_operator Ah0, Ps0, Rg;
  flow_operator Cg;             /* mg->C[0] restricted to the owned columns
                                   (column index minus r0); rowptr NULL: the
                                   three-collective form */
  const int* up_rowblocks0;     /* mg->up_rowblocks[0] for the owned rows */
  int up_nblocks0;
  /* ONE collective per iteration (two-collective form only): z_hi > z_lo --
   * up_rowblocks0 then covers the rows [z_lo, z_hi) = the owned rows plus ONE
   * ghost layer, and the flow_rows handed to the solver reach TWO layers out:
   * the halo of w (in the collective that carries the dots) is two layers
   * deep, so r is current two layers out, so the up-sweep can form z on the
   * first ghost layer itself -- every rank recomputing those few rows instead
   * of asking for them -- and w = A z needs no halo of z.  x comes back on
   * [z_lo, z_hi). */
  int z_lo, z_hi;
} flow_mg_shard;
int flow_shard_mgcg_solve(const flow_comm* comm, const flow_rows* rows,
                          const flow_operator* A, const double* dinv,
                          const flow_mg_shard* mgs, const double* b, double* x,
                          double rtol, double atol, int maxit, int check_every,
                          int first_check, double* work, size_t work_len,
                          int* iters_host, double* resid_host,
                          int* start_rejected_host, void* stream);

/* The mass solver of K18 on the strips.  A correction's polynomial reaches
 * steps - 1 matrix hops: with the scaled defect known on a ghost zone `steps`
 * vertex columns deep the rank computes product j on the rows within
 * steps - 1 - j hops of its own (rowblocks16[j]: CSR-stream row blocks of that
 * row range, <= FLOW_PMG_NNZ_PER_BLOCK nonzeros each, global row numbers) and
 * ends with x advanced on its own rows and its first ghost layer (the rows
 * [row_lo_last, row_hi_last) of the last product) -- no communication inside a
 * correction, ONE collective per correction: the deep halo of the defect with
 * the norms of the correction before riding along (so a solve that needs m
 * corrections issues m + 1).  `rows`: the owned rows with the DEEP ghost range
 * [e0, e1) and its halo slots; M->A: the operator with the row blocks of the
 * owned rows; M->work16: 5 * ncomp * (e1 - e0) floats (work16_rows = e1 - e0);
 * the plain fp16 stream M->vals16 is used (the packed one is tiled once).
 * xbase != NULL: the increment form (b = the defect of xbase; delta0 or NULL
 * as flow_mass_solve_increment; x = xbase + increment on the rows of the last
 * product); xbase == NULL: x holds the start, valid on own + first ghost rows.
 * work: FLOW_REDUCE_WORK + 2 * nblocks16[last] + 1 [+ op size] doubles. */
typedef struct {
  int nlevels;                    /* = steps - 1 */
  const int* rowblocks16[16];
  int nblocks16[16];
  int row_lo_last, row_hi_last;
} flow_mass_strips;
int flow_shard_mass_solve(const flow_comm* comm, const flow_rows* rows,
                          const flow_mass* M, const flow_mass_strips* levels,
                          const double* b, const double* xbase,
                          const double* delta0, double* x, double rtol,
                          double atol, int maxit, int first_check, double* work,
                          size_t work_len, int* iters_host, double* resid_host,
                          void* stream);

/* GMRES(restart) on the strips: for the Newton systems -- the operator is the
 * matrix-free Jacobian action (kind 3) whose flow_mesh / flow_space carry the
 * rank's cell and row ranges (below) -- and for scalar systems (kind 0 with the
 * row blocks of the owned rows, one component: the heat system,
 * flow/heat.py:103-122; verify as flow_gmres_solve).  The preconditioner is
 * block Jacobi, no
 * communication: EITHER ilu, the factors of the rank's own diagonal block (plan
 * over the owned rows in local numbering), OR pmg, the two-level cycle of K17
 * on that block (levels in local numbering, flow_pmg_pack).  The Krylov vectors hold the owned rows only
 * (2 * (r1 - r0) doubles); per iteration one halo collective (the operator's
 * input) and one for the dot products, whose sums the device-side step of
 * flow_gmres_solve takes straight from the exchange buffer: no read-back per
 * iteration here either (expected_its as there; every rank must pass the same
 * value -- it decides how many collectives are enqueued).  b, x: global-length
 * fields (owned rows).  work: FLOW_REDUCE_WORK + (2*restart + 4) * 2*(r1-r0)
 * + 2*(e1-e0) + FLOW_GMRES_PARTIALS + FLOW_GMRES_STATE doubles. */
int flow_shard_gmres_solve(const flow_comm* comm, const flow_rows* rows,
                           const flow_operator* A, const flow_ilu* ilu,
                           const flow_pmg* pmg, const double* b, double* x,
                           double rtol, double atol,
                           int maxit, int restart, int x_is_zero,
                           int expected_its, int verify, double* work,
                           size_t work_len, int* iters_host, double* resid_host,
                           void* stream);

/* ---- assembly ------------------------------------------------------------
 * Two-phase, atomic-free: a cell kernel writes local tensors to `scratch`
 * ([entry][cell]); a gather kernel sums, per CSR nonzero / per dof, the
 * contributions listed in the contribution maps built once per mesh on the
 * host (flow_amd/fem/space.py). */
typedef struct {
  int nc;                  /* cells */
  const double* xy;        /* (2,3,nc): vertex coordinates */
  int c0, c1;              /* K15: the cell kernels run over [c0, c1) only
                              (c1 = 0: all cells) -- a rank's cells are those
                              that touch its owned rows */
} flow_mesh;

typedef struct {
  int deg;                 /* 1 | 2 */
  int n;                   /* scalar dofs */
  int nnz;
  const int* cell_dofs;    /* (nloc, nc) */
  const int* cptr;         /* nnz+1  matrix contribution map */
  const int* csrc;
  const int* vptr;         /* n+1    vector contribution map */
  const int* vsrc;
  int r0, r1;              /* K15: the gathers fill the rows [r0, r1) only
                              (r1 = 0: all rows) ... */
  int nnz0, nnz1;          /* ... and the nonzeros [nnz0, nnz1) = [rowptr[r0],
                              rowptr[r1]) of matrix planes */
} flow_space;

/* per-cell P_k lattice values of a coefficient (Constant / Expression(degree=k)
 * / Function), `dim` components: values[(a*nl + l)*nc_eff + c*cell_stride];
 * G = (nl x nloc_test) reference matrix int psi_l phi_i. */
typedef struct {
  int nl;
  int cell_stride;         /* 0: spatially constant, 1: per cell */
  const double* values;
  const double* G;
} flow_coef;

/* K1: a2 = dot(grad(p), grad(q))*dx            (pressure_correction.py:317)
 * K3: a3 = inner(u2, v)*dx per component       (pressure_correction.py:442)
 * kind 0: stiffness, 1: mass, 2: vertex-quadrature lumped mass (heat.py:39-45).
 * scratch: nloc^2 * nc doubles. */
int flow_assemble_scalar_matrix(int kind, const flow_mesh* mesh,
                                const flow_space* V, double* scratch,
                                double* vals, void* stream);

/* K2: L2 (pressure_correction.py:318-323):
 *   b_i = -alpha*rho/dt (div u, q_i) + (grad p0, grad q_i)
 *         [- mu (grad div u, grad q_i)  if rotational].
 * W: velocity scalar space (deg 1|2), P: P1.  scratch: 3*nc. */
int flow_assemble_pressure_rhs(const flow_mesh* mesh, const flow_space* W,
                               const flow_space* P, const double* u,
                               const double* p0, double alpha_rho_dt, double mu,
                               int rotational, double* scratch, double* b,
                               void* stream);

/* K4: L3 (pressure_correction.py:444-449):
 *   b_(a,i) = (u_a, v_i) - dt/rho (d_a phi, v_i),
 *   phi = p1 - p0 [+ mu div u  if rotational & 1].   scratch: 2*nloc*nc.
 * rotational & 2: WITHOUT the (u_a, v_i) term -- the defect b - M u of the
 * start u = ui, the right-hand side of the correction's increment
 * (flow_mass_solve_increment). */
int flow_assemble_correction_rhs(const flow_mesh* mesh, const flow_space* W,
                                 const flow_space* P, const double* u,
                                 const double* p1, const double* p0,
                                 double dt_rho, double mu, int rotational,
                                 double* scratch, double* b, void* stream);

/* K5+K6: F1 and J = derivative(F1, ui) (pressure_correction.py:169-202) with
 * the integrand of _rhs_weak (:135-144), exterior-facet terms included:
 *   F = (ui - u0, v) - dt/rho [theta_i R(ui; f1) + theta_e R(u0; f0)],
 *   J = dF/dui.
 * bfmask[c]: bit i set iff local facet i of cell c is a boundary facet.
 * F (2n) and/or Jvals (4 planes, j_plane_stride >= nnz apart) may be NULL to
 * skip.
 * scratch: max(2*nloc, 4*nloc^2) * nc doubles. */
typedef struct {
  double dt, rho, mu, theta_i, theta_e;
} flow_ns_params;
int flow_assemble_momentum(const flow_mesh* mesh, const flow_space* W,
                           const flow_space* P, const int* bfmask,
                           const double* ui, const double* u0,
                           const double* p0, const flow_coef* f0,
                           const flow_coef* f1, const flow_ns_params* prm,
                           double* scratch, double* F, double* Jvals,
                           size_t j_plane_stride, void* stream);

/* Matrix-free action of that Jacobian, out = J(ui) v = dF1/dui [v] (the
 * directional derivative of the form, evaluated cell by cell like the residual;
 * `derivative(F1, ui)` applied instead of assembled, pressure_correction.py:202):
 * costs what the assembled 2x2-block SpMV costs and makes the per-Newton-step
 * Jacobian assembly unnecessary -- the assembled diagonal blocks are then only
 * needed when the (lagged) ILU(0) is refactored.  Rows of the nbc Dirichlet
 * dofs are identity rows (out[d] = v[d]), as flow_bc_identity_rows makes them.
 * scratch: 2*nloc*nc doubles, private to this operator while a solve runs.
 * A flow_operator of kind 3 carries a pointer to this struct in `matfree`. */
typedef struct {
  const flow_mesh* mesh;
  const flow_space* W;       /* velocity space, needs vptr/vsrc */
  const int* bfmask;         /* nc: exterior-facet bits (as flow_assemble_momentum) */
  const double* ui;          /* 2*W->n: linearisation point */
  flow_ns_params prm;
  double* scratch;
  int nbc;
  const int* bc_dofs;        /* nbc Dirichlet dofs (component-blocked numbering) */
  const unsigned char* bc_mask;   /* 2n bytes, 1 on those dofs, or NULL: with it
                                     the gather writes the identity rows itself
                                     (one launch less per application) */
} flow_momentum_jvp;
int flow_momentum_jvp_apply(const flow_momentum_jvp* J, const double* v,
                            double* out, void* stream);

/* (f, v) for a `dim`-component coefficient: the load vector behind
 * dolfin.project (tests/test_navier_stokes.py:296-308).  scratch: dim*nloc*nc. */
int flow_assemble_source(const flow_mesh* mesh, const flow_space* V, int dim,
                         const flow_coef* f, double* scratch, double* b,
                         void* stream);

/* Stokes bootstrap (flow/stokes.py:40-42): adjoint of the
 * divergence coupling, out_(a,i) = - int p d_a phi_i  (`- p*div(v)*dx`); the
 * coupling itself, - int q div u, is flow_assemble_pressure_rhs with p0 = 0,
 * alpha_rho_dt = 1.  scratch: 2*nloc*nc. */
int flow_assemble_div_adjoint(const flow_mesh* mesh, const flow_space* W,
                              const flow_space* P, const double* p,
                              double* scratch, double* out, void* stream);

/* K16: b_i = int m(u) phi_i with m = sqrt(ux^2+uy^2) (mode 0) or |ux|+|uy|
 * (mode 1): the load vector of the callers' `project(sqrt(ux**2 + uy**2), ...)`
 * step-size control (tests/test_karman_vortex_street.py:262-268,
 * tests/test_boussinesq.py:268-273).  scratch: nloc*nc. */
int flow_assemble_magnitude(const flow_mesh* mesh, const flow_space* W, int mode,
                            const double* u, double* scratch, double* b,
                            void* stream);

/* ---- forms: integrals of expressions of fields (flow_amd/fem/forms.py) -----
 * The host expands a UFL-style integrand into scalar trees and compiles each
 * to a register program: at most FLOW_FORM_MAX_PROGRAM instructions
 * (op, dst, a, b) over FLOW_FORM_REGISTERS fp64 registers r[0..7].  A cell
 * kernel runs the program at every point of the quadrature rule; `out` ops
 * hand a register to output 0 or 1 (to a coefficient slot in the programs of
 * flow_form_matrix / flow_form_vector).
 *   const  r[dst] = consts[a]          coord  r[dst] = x_a at the point
 *   field  r[dst] = field a (b = 0), d/dx (b = 1) or d/dy (b = 2)
 *   expr   r[dst] = sum_l expr[a][l][c] * tables[expr_table[a] + q*nl + l]
 *   mov    r[dst] = r[a]               add sub mul div pow  r[dst] = r[a] o r[b]
 *   neg abs sqrt exp ln sin cos  r[dst] = f(r[a])
 *   out    output b = r[a]
 *   normal r[dst] = component a of the outward unit normal (facet
 *          integrals only: the cell entry points refuse it)
 *   lt le eq ne  r[dst] = r[a] o r[b] ? 1.0 : 0.0
 *   select r[dst] = r[a] != 0 ? r[b] : r[dst]   (the value not selected is
 *          not read: an inf or NaN in it does not reach the result)
 *   min max  r[dst] = the smaller | larger of r[a], r[b] (fmin / fmax: where
 *          one operand is NaN the OTHER is returned -- numpy.minimum /
 *          maximum and UFL's conditional-based definition give NaN there;
 *          `Or` of two conditions is max of their 0-1 values, never NaN)
 *   sign   r[dst] = -1, 0, 1 by the sign of r[a]; +-0 and NaN are returned as
 *          they are                                   tanh  r[dst] = tanh r[a]
 *   cell   r[dst] = a = 0: |T|, 1: the circumradius, 2: the diameter (largest
 *          vertex distance) of the cell (of the owning cell on facets and at
 *          points), from the vertex coordinates the kernels hold
 * The program and the constants travel by value with the launch (constants
 * may change from call to call at no cost); rule and tables are device
 * arrays, uploaded once per program signature and degree by the host. */
#define FLOW_FORM_MAX_PROGRAM 64
#define FLOW_FORM_REGISTERS 8
#define FLOW_FORM_MAX_CONSTANTS 32
#define FLOW_FORM_MAX_FIELDS 6
#define FLOW_FORM_MAX_EXPRESSIONS 4
#define FLOW_FORM_MAX_POINTS 256
#define FLOW_FORM_SLOTS 9     /* coefficient slots of a rank-2 form */
#define FLOW_FORM_NEWTON_SLOTS 12   /* those, then the 3 of a rank-1 form */
#define FLOW_FORM_OP_CONST 0
#define FLOW_FORM_OP_COORD 1
#define FLOW_FORM_OP_FIELD 2
#define FLOW_FORM_OP_EXPR 3
#define FLOW_FORM_OP_MOV 4
#define FLOW_FORM_OP_ADD 5
#define FLOW_FORM_OP_SUB 6
#define FLOW_FORM_OP_MUL 7
#define FLOW_FORM_OP_DIV 8
#define FLOW_FORM_OP_POW 9
#define FLOW_FORM_OP_NEG 10
#define FLOW_FORM_OP_ABS 11
#define FLOW_FORM_OP_SQRT 12
#define FLOW_FORM_OP_EXP 13
#define FLOW_FORM_OP_LN 14
#define FLOW_FORM_OP_SIN 15
#define FLOW_FORM_OP_COS 16
#define FLOW_FORM_OP_OUT 17
#define FLOW_FORM_OP_NORMAL 18
#define FLOW_FORM_OP_LT 19
#define FLOW_FORM_OP_LE 20
#define FLOW_FORM_OP_EQ 21
#define FLOW_FORM_OP_NE 22
#define FLOW_FORM_OP_SELECT 23
#define FLOW_FORM_OP_MIN 24
#define FLOW_FORM_OP_MAX 25
#define FLOW_FORM_OP_SIGN 26
#define FLOW_FORM_OP_TANH 27
#define FLOW_FORM_OP_CELL 28
/* Interior facets (flow_form_interior_facet_*): a lane holds the two cells of
 * its facet, '+' (the smaller cell index) and '-'.  The leaf instructions carry
 * a side bit -- clear '+', set '-' -- in an operand bit the other entry points
 * keep at zero (they refuse it): FIELD in b beside the derivative, NORMAL in a
 * beside the component, CELL in a beside the quantity.  Every (field,
 * component, side) is a field slot of its own, loaded from the cell of its
 * side; a slot is read on one side only.  COORD is the point itself.
 *   facet_len  r[dst] = the length of the facet (interior facets only)
 * A program without a side bit and without facet_len is what it always was. */
#define FLOW_FORM_OP_FACET_LEN 29
#define FLOW_FORM_SIDE_FIELD 4
#define FLOW_FORM_SIDE_NORMAL 2
#define FLOW_FORM_SIDE_CELL 4
typedef struct {
  int nprog;
  int prog[4 * FLOW_FORM_MAX_PROGRAM];     /* (op, dst, a, b) per instruction */
  int nconst;
  double consts[FLOW_FORM_MAX_CONSTANTS];
  int nfield;                              /* scalar field components */
  const double* field[FLOW_FORM_MAX_FIELDS];   /* n dofs each */
  int field_deg[FLOW_FORM_MAX_FIELDS];     /* 1 | 2 */
  const int* cell_dofs[2];                 /* (nloc, nc) of the P1 | P2 layout */
  int nexpr;                               /* Expression components */
  const double* expr[FLOW_FORM_MAX_EXPRESSIONS];   /* P_k lattice (nl, nc) */
  int expr_nl[FLOW_FORM_MAX_EXPRESSIONS];  /* nl <= 21 (k <= 5) */
  int expr_table[FLOW_FORM_MAX_EXPRESSIONS];
  int nq;                                  /* <= FLOW_FORM_MAX_POINTS */
  const double* rule;                      /* nq x 3: xi, eta, weight (sum 1/2) */
  const double* tables;                    /* P_k basis at the rule's points */
  int ntables;                             /* doubles in tables */
  int nout;                                /* 1 | 2; flow_form_matrix: 9,
                                              flow_form_vector: 3,
                                              flow_form_newton: 12 */
} flow_form;

/* assemble(f*dx): the integral of output 0 over the cells of `mesh`, to the
 * host.  Fixed-order reduction (per-cell integrals, <= 1024 block partials,
 * one finishing block): bitwise reproducible.  scratch: nc doubles; work:
 * FLOW_REDUCE_WORK doubles. */
int flow_form_functional(const flow_mesh* mesh, const flow_form* form,
                         double* scratch, double* work, double* result_host,
                         void* stream);

/* Stage 1 of flow_form_functional alone: out[c] = the integral of output 0
 * over cell c (device, nc doubles), not summed.  Enqueued; nothing
 * synchronises.  Not on strips. */
int flow_form_cell_values(const flow_mesh* mesh, const flow_form* form, double* out,
                          void* stream);

/* assemble(f*ds): the integral of output 0 over a list of exterior facets,
 * facet k being local facet facet_local[k] (the edge opposite that vertex)
 * of cell facet_cell[k] (device int32 arrays of nfacets entries).  The rule
 * holds 3*nq rows: the nq points of local facet 0, then 1, then 2, in
 * reference coordinates, weights summing to 1 per facet (scaled by the
 * facet's length); the Expression tables hold 3*nq rows to match.  Fixed-order
 * reduction as flow_form_functional: bitwise reproducible.  nfacets == 0:
 * 0.0, nothing launched.  Not on strips.  scratch: nfacets doubles; work:
 * FLOW_REDUCE_WORK doubles. */
int flow_form_facet_functional(const flow_mesh* mesh, const flow_form* form,
                               int nfacets, const int* facet_cell,
                               const int* facet_local, double* scratch,
                               double* work, double* result_host, void* stream);

/* Wall distributions (flow_amd/fem/profile.py, BoundaryProfile): the program
 * at every sample of every listed exterior facet, not reduced.  The rule is
 * that of flow_form_facet_functional (3*nq rows, m = nq samples per facet);
 * one lane per (facet, sample), nfacets*m lanes: a boundary holds O(sqrt(N))
 * facets, so the samples are the parallelism.  Lane (k, j) computes the
 * facet's normal and length as the facet functional does, runs the program at
 * row facet_local[k]*m + j and writes output o < nout (1 | 2) to
 *     values[o*npoints + facet_dest[k]*m + j'],   npoints = nfacets*m,
 * j' = m-1-j where facet_flip[k] != 0, else j: with facet_dest the facet's
 * position along its boundary curve and facet_flip set where the curve runs
 * against the facet's own direction (from vertex facet_v0 to facet_v1), the
 * samples arrive in arclength order and no permutation pass follows.
 * integrals != NULL: lane j == 0 also writes the facet's integral of output o
 * to integrals[o*nfacets + facet_dest[k]], summed over the m rows with the
 * arithmetic and the order of the facet functional's per-facet value (the same
 * bits).  facet_cell, facet_local, facet_dest, facet_flip: device int32 arrays
 * of nfacets entries; facet_dest must be a permutation of 0..nfacets-1, which
 * the caller checks (a destination outside 0..nfacets-1 is skipped, a
 * repeated one leaves entries unwritten).  A facet whose cell or local index
 * is out of range gives NaN in its samples and its integral.  values:
 * nout*npoints doubles; integrals: nout*nfacets doubles or NULL.  nfacets ==
 * 0: nothing launched.  No atomics: two calls give the same bits.  Not on
 * strips. */
int flow_form_facet_values(const flow_mesh* mesh, const flow_form* form,
                           int nfacets, const int* facet_cell,
                           const int* facet_local, const int* facet_dest,
                           const int* facet_flip, double* values,
                           double* integrals, void* stream);

/* assemble(f*dS): the integral of output 0 over a list of interior facets.
 * Facet k is local facet local_plus[k] of its '+' cell facet_plus[k] and
 * local facet j of its '-' cell n, with facet_other[k] = (n << 3) | (j << 1) |
 * flip, flip = 0 where the first vertex of the facet in '-' is its first
 * vertex in '+' (the vertices of local facet i are i == 0 ? 1 : 0 and i == 2 ?
 * 1 : 2) and 1 where it is the second: what adapt.facet_table packs (device
 * int32 arrays of nfacets entries).  One lane per facet walks the rows of
 * local facet local_plus[k] of the rule (that of flow_form_facet_functional, 3*nq
 * rows), runs the program once per point and scales by the facet's length in
 * the '+' cell.  A leaf with its side bit set is evaluated on the '-' cell:
 * barycentric coordinates zero at vertex j, the '+' facet's pair on the other
 * two (swapped where flip is set), the normal that of the '-' cell itself.
 * EXPR is refused.  An entry outside the mesh gives NaN for that facet.
 * Fixed-order reduction as flow_form_functional, no atomics: bitwise
 * reproducible.  nfacets == 0: 0.0, nothing launched.  Not on strips.
 * scratch: nfacets doubles (scratch[k] = the integral over facet k); work:
 * FLOW_REDUCE_WORK doubles. */
int flow_form_interior_facet_functional(const flow_mesh* mesh, const flow_form* form,
                                        int nfacets, const int* facet_plus,
                                        const int* local_plus, const int* facet_other,
                                        double* scratch, double* work,
                                        double* result_host, void* stream);

/* The same launch without the sum: out[k] = the integral over facet k (device,
 * nfacets doubles).  Enqueued; nothing synchronises. */
int flow_form_interior_facet_values(const flow_mesh* mesh, const flow_form* form,
                                    int nfacets, const int* facet_plus,
                                    const int* local_plus, const int* facet_other,
                                    double* out, void* stream);

/* Per-cell shares of per-facet values: one lane per cell c,
 *     out[c] = share * sum_{i = 0, 1, 2} values[position[i*nc + c]],
 * always in the order i = 0, 1, 2, with position[i*nc + c] the index in
 * `values` of local facet i of cell c (the edge -> position map of a facet
 * selection, gathered through the cell's edges on the host) or -1 (a boundary
 * facet, or one not selected), which is skipped.  position: device int32,
 * 3*nc; values: device, nfacets doubles; out: device, nc doubles.  No atomics. */
int flow_facet_cell_shares(const flow_mesh* mesh, int nfacets, const int* position,
                           const double* values, double share, double* out,
                           void* stream);

/* Running integrals along boundary curves: for every curve c < ncurves and
 * row r < nrows, out[r*nfacets + k] = integrals[r*nfacets + b] + ... +
 * integrals[r*nfacets + k] for b = curve_facets[c] <= k < curve_facets[c+1],
 * restarting at every curve.  One lane per (curve, row) adds strictly left to
 * right: boundaries hold thousands of facets, not millions, and the fixed
 * order is the point of this entry -- a sequential sum on the host
 * (numpy.cumsum) gives the same bits, which no scan tree does.  curve_facets:
 * HOST array of ncurves + 1 offsets, 0 first, nfacets last, non-decreasing
 * (checked here; they travel with the launches by value,
 * FLOW_PROFILE_CURVES_PER_LAUNCH curves each).  integrals, out: device,
 * nrows*nfacets doubles, two different arrays. */
#define FLOW_PROFILE_CURVES_PER_LAUNCH 32
int flow_profile_cumsum(int ncurves, const int* curve_facets, int nrows,
                        int nfacets, const double* integrals, double* out,
                        void* stream);

/* Load vector b_(o,i) = int out_o phi_i for o < form->nout (the right-hand
 * side of project(f, V)); V: test space (deg 1|2).  scratch: nout*nloc*nc. */
int flow_form_load_vector(const flow_mesh* mesh, const flow_space* V,
                          const flow_form* form, double* scratch, double* b,
                          void* stream);

/* Forms of a test function v and a trial function u of the scalar space V
 * (TestFunction / TrialFunction of forms.py).  The host rewrites the integrand
 * by linearity as  sum_(b,a) c_ba D_a u D_b v  (rank 2) or  sum_b c_b D_b v
 * (rank 1), D_0 the value, D_1 d/dx, D_2 d/dy, and compiles the argument-free
 * coefficients into one program: `out` slot 3 b + a holds c_ba (nout =
 * FLOW_FORM_SLOTS), slot b holds c_b (nout = 3).  Slots the program does not
 * write are absent terms (a bit mask of the written ones travels with the
 * launch); at least one must be written, none twice; NORMAL is refused.
 *   flow_form_matrix: Ke[i][j] = sum_q w_q |det J| sum_ba c_ba(x_q) D_a phi_j
 *     D_b phi_i per cell, summed over cptr / csrc into `vals`, one value plane
 *     (nnz doubles) of a kind-0 operator on V's pattern.  scratch: nloc^2 * nc.
 *   flow_form_vector: b_i = sum_q w_q |det J| sum_b c_b(x_q) D_b phi_i, summed
 *     over vptr / vsrc into b (n doubles).  scratch: nloc * nc.
 * No floating-point atomics: two calls give the same bits.  Not on strips. */
int flow_form_matrix(const flow_mesh* mesh, const flow_space* V,
                     const flow_form* form, double* scratch, double* vals,
                     void* stream);
int flow_form_vector(const flow_mesh* mesh, const flow_space* V,
                     const flow_form* form, double* scratch, double* b,
                     void* stream);

/* The Jacobian J(u) and the residual F(u) of a Newton iteration in one pass
 * over the cells: ONE program holds both coefficient tables, slot 3 b + a the
 * Jacobian's c_ba and slot FLOW_FORM_SLOTS + b the residual's c_b (nout =
 * FLOW_FORM_NEWTON_SLOTS; at least one slot of each must be written, none
 * twice), so geometry, field values, basis tables and the subexpressions the
 * two tables share are loaded and computed once per quadrature point.  Ke and
 * be are accumulated as flow_form_matrix and flow_form_vector accumulate them
 * and gathered over cptr / csrc into `vals` (nnz doubles) and over vptr / vsrc
 * into b (n doubles).  No floating-point atomics: two calls give the same
 * bits.  Not on strips.  scratch: (nloc^2 + nloc) * nc. */
int flow_form_newton(const flow_mesh* mesh, const flow_space* V,
                     const flow_form* form, double* scratch, double* vals,
                     double* b, void* stream);

/* Forms of arguments over exterior facets (Neumann, Robin and Nitsche terms:
 * g*v*ds, h*u*v*ds, dot(grad(u), n)*v*ds).  The program is a coefficient
 * table as for flow_form_matrix (nout = FLOW_FORM_SLOTS) / flow_form_vector
 * (nout = 3) in which NORMAL is legal; the rule, the Expression tables and the
 * facet lists are those of flow_form_facet_functional (3*nq rows).
 *   Element kernel: one lane per (local test dof i < nloc, facet k), k
 * fastest, nloc*nfacets lanes.  All nloc basis functions of the owning cell
 * take part.  Lane (i, k) writes row i of the facet's element matrix to
 *     scratch[(i*nloc + j)*nfacets + k]   (matrix; scratch: nloc^2 * nfacets)
 * or entry i of its element vector to
 *     scratch[i*nfacets + k]              (vector; scratch: nloc * nfacets),
 * accumulated per point as flow_form_matrix / flow_form_vector do, with w =
 * rule weight x facet length.  A facet whose cell or local index is out of
 * range gives NaN.
 *   Gather: one lane per target t < ntargets adds scratch[map_src[e]] for e in
 * [map_ptr[t], map_ptr[t+1]) in that order and writes out[map_targets[t]]
 * (targets: indices of nonzeros of V's CSR pattern | dofs); EVERY OTHER ENTRY
 * OF THE OUTPUT IS LEFT AS IT IS, so the caller passes a zeroed buffer once
 * and may reuse it while the map stays the same.  A target outside the output
 * is skipped, a map row or source outside the scratch gives NaN.  map_targets
 * (ntargets), map_ptr (ntargets + 1), map_src (all scratch entries): device
 * int32 arrays the host builds once per (facet selection, space).  nfacets ==
 * 0 or ntargets == 0: nothing launched.  No atomics: two calls give the same
 * bits.  Not on strips. */
int flow_form_facet_matrix(const flow_mesh* mesh, const flow_space* V,
                           const flow_form* form, int nfacets,
                           const int* facet_cell, const int* facet_local,
                           int ntargets, const int* map_targets,
                           const int* map_ptr, const int* map_src,
                           double* scratch, double* vals, void* stream);
int flow_form_facet_vector(const flow_mesh* mesh, const flow_space* V,
                           const flow_form* form, int nfacets,
                           const int* facet_cell, const int* facet_local,
                           int ntargets, const int* map_targets,
                           const int* map_ptr, const int* map_src,
                           double* scratch, double* b, void* stream);

/* Cell subdomains (assemble(f*dx(k)), forms.cell_subdomains): the integrals of
 * flow_form_functional / flow_form_cell_values / flow_form_matrix /
 * flow_form_vector over a LIST of cells.  cells: device int32 (ncells), the
 * selected cells; the program, the rule and the Expression tables are those of
 * the whole-mesh entry point (1 * nq rows, no NORMAL).  Lane k takes cell
 * cells[k] and runs the whole-mesh kernel's arithmetic on it: a list that
 * holds every cell in ascending order gives the whole-mesh entry point's bits.
 * A list entry outside [0, nc) gives NaN (cells_values: it is skipped).
 *   flow_form_cells_functional: per-cell integrals to scratch[k] (ncells
 * doubles), then the fixed-order reduction of flow_form_functional over
 * [0, ncells) (work: FLOW_REDUCE_WORK doubles) into *result_host.
 *   flow_form_cells_values: out[cells[k]] = the integral over that cell; every
 * other entry of out (nc doubles) is left as it is: the caller zeroes it.
 *   flow_form_cells_matrix / flow_form_cells_vector: lane k writes the element
 * matrix of its cell to scratch[(i*nloc + j)*ncells + k] (scratch: nloc^2 *
 * ncells) or its element vector to scratch[i*ncells + k] (nloc * ncells); the
 * gather of flow_form_facet_matrix then sums them over (map_targets, map_ptr,
 * map_src) into vals (nnz) / b (n) and leaves every other entry as it is.  For
 * the bits of the whole-mesh entry point the sources of a target stand in the
 * order of V's own cptr / csrc (vptr / vsrc) restricted to the list
 * (ops.cell_map_host).
 * ncells == 0 (or ntargets == 0): FLOW_OK, nothing launched (the functional:
 * *result_host = 0.0).  No atomics: two calls give the same bits.  Not on
 * strips. */
int flow_form_cells_functional(const flow_mesh* mesh, const flow_form* form,
                               int ncells, const int* cells, double* scratch,
                               double* work, double* result_host, void* stream);
int flow_form_cells_values(const flow_mesh* mesh, const flow_form* form,
                           int ncells, const int* cells, double* out,
                           void* stream);
int flow_form_cells_matrix(const flow_mesh* mesh, const flow_space* V,
                           const flow_form* form, int ncells, const int* cells,
                           int ntargets, const int* map_targets,
                           const int* map_ptr, const int* map_src,
                           double* scratch, double* vals, void* stream);
int flow_form_cells_vector(const flow_mesh* mesh, const flow_space* V,
                           const flow_form* form, int ncells, const int* cells,
                           int ntargets, const int* map_targets,
                           const int* map_ptr, const int* map_src,
                           double* scratch, double* b, void* stream);

/* Rectangular blocks: a test function of the scalar space V_test and a trial
 * function of the scalar space V_trial on one mesh (degrees 1 | 2, equal or
 * not) -- the velocity-pressure coupling of a form on a Taylor-Hood space
 * (forms.py, mixed_arguments).  The program is the coefficient table of
 * flow_form_matrix (nout = FLOW_FORM_SLOTS: slot 3 b + a multiplies D_a of the
 * trial and D_b of the test function); the rule and the tables are those of
 * flow_form_matrix (rect_matrix, rect_cells_matrix) or of
 * flow_form_facet_matrix (rect_facet_matrix: 3*nq rows, NORMAL legal).
 *   Element kernels: flow_form_matrix's, flow_form_facet_matrix's and
 * flow_form_cells_matrix's with two bases -- per point and test derivative b,
 * t_j = sum_a w c_ba D_a psi_j over the trial basis first, then Ke[i][j] +=
 * D_b phi_i t_j over the test basis -- into
 *     scratch[(i*nloc_trial + j)*n + k],  n = nc | nfacets | ncells, k fastest
 * (scratch: nloc_test * nloc_trial * n doubles).
 *   flow_form_rect_matrix: the gather sums scratch over cptr (nnz + 1) / csrc
 * in order into vals (nnz doubles), the pattern of pairs (test dof, trial dof)
 * that share a cell (space.RectLayout).  With V_test == V_trial and the maps
 * of that space it gives the bits of flow_form_matrix.
 *   flow_form_rect_facet_matrix / flow_form_rect_cells_matrix: the gather of
 * flow_form_facet_matrix over (map_targets, map_ptr, map_src) into vals (nnz);
 * every other entry is left as it is.  nfacets | ncells == 0 or ntargets == 0:
 * nothing launched.
 *   Refused: degrees outside {1, 2}, a space with more dofs than the cells of
 * the mesh can hold (a space of another mesh), NORMAL in the two cell entry
 * points, strips, nnz above the scratch entries or above n_test * n_trial,
 * more targets than nnz.  A map row or source outside the scratch, a list
 * entry outside the mesh: NaN, not a stray read.  No atomics: two calls give
 * the same bits. */
int flow_form_rect_matrix(const flow_mesh* mesh, const flow_space* V_test,
                          const flow_space* V_trial, const flow_form* form,
                          double* scratch, double* vals, const int* cptr,
                          const int* csrc, int nnz, void* stream);
int flow_form_rect_facet_matrix(const flow_mesh* mesh, const flow_space* V_test,
                                const flow_space* V_trial, const flow_form* form,
                                int nfacets, const int* facet_cell,
                                const int* facet_local, int ntargets,
                                const int* map_targets, const int* map_ptr,
                                const int* map_src, double* scratch, double* vals,
                                int nnz, void* stream);
int flow_form_rect_cells_matrix(const flow_mesh* mesh, const flow_space* V_test,
                                const flow_space* V_trial, const flow_form* form,
                                int ncells, const int* cells, int ntargets,
                                const int* map_targets, const int* map_ptr,
                                const int* map_src, double* scratch, double* vals,
                                int nnz, void* stream);
/* vals[e] = 0 for every entry e of a rectangular CSR plane (rowptr: n_rows + 1)
 * whose row (row_isbc, n_rows bytes) or column (col_isbc, one byte per column)
 * is a Dirichlet dof; the other entries stay.  One lane per row. */
int flow_bc_rect_mask(const int* rowptr, const int* cols, int n_rows, double* vals,
                      const unsigned char* row_isbc, const unsigned char* col_isbc,
                      void* stream);

/* Forms of a test function v and a trial function u of the VECTOR space on V's
 * scalar pattern (forms.py, vector_arguments): the host rewrites the integrand
 * as  sum_(r,s) sum_(b,a) c^rs_ba D_a u_s D_b v_r  (rank 2) or  sum_r sum_b
 * c^r_b D_b v_r  (rank 1) and compiles the table of every block that has a
 * term into the program(s) of a scalar form, as for flow_form_matrix /
 * flow_form_vector.  forms: nprog (1..64) structs behind one another;
 * blocks[k]: the block of program k, p = 2 r + s in 0..3 (matrix) or r in 0..1
 * (vector), r the test and s the trial component -- host arrays.
 *   Every program runs on the element kernel of flow_form_matrix /
 * flow_form_vector, with its arithmetic, into the scratch plane of its block;
 * a further program of a block is added to the plane entry by entry.  ONE
 * gather over cptr / csrc (vptr / vsrc) then sums the planes of all blocks:
 *   flow_form_block_matrix: vals + p*plane_stride, p = 0..3, the four value
 *     planes of a kind-2 operator (plane_stride >= nnz doubles apart);
 *   flow_form_block_vector: b[r*n + i], 2n doubles, component-major.
 * The plane or component of a block without a program is set to zero.  A
 * block whose only program is that of a scalar form gets the bits
 * flow_form_matrix / flow_form_vector give that form.  No floating-point
 * atomics: two calls give the same bits.  Not on strips.
 * scratch: (blocks with a program, + 1 where one has several) * nloc^2 * nc
 * doubles (matrix; vector: * nloc * nc). */
int flow_form_block_matrix(const flow_mesh* mesh, const flow_space* V, int nprog,
                           const flow_form* forms, const int* blocks,
                           double* scratch, double* vals, size_t plane_stride,
                           void* stream);
int flow_form_block_vector(const flow_mesh* mesh, const flow_space* V, int nprog,
                           const flow_form* forms, const int* blocks,
                           double* scratch, double* b, void* stream);

/* The Jacobian (a 2x2-block form) and the residual (2 components) of a Newton
 * iteration on the VECTOR space on V's scalar pattern, at one state, in one
 * call (forms.py, vector_derivatives; ops.py, NewtonAssembler).  forms: nprog
 * (1..64) structs behind one another; kinds[k], tags[k] (host arrays):
 *   FLOW_BLOCK_NEWTON, p: the program of flow_form_newton (nout =
 *     FLOW_FORM_NEWTON_SLOTS) for block p = 2 r + s together with residual
 *     component r = p / 2, on its element kernel: Ke to the block's scratch
 *     plane, be directly behind it.  It must be the first program of its block
 *     and of its component;
 *   FLOW_BLOCK_MATRIX, p: a program of flow_form_block_matrix for block p;
 *   FLOW_BLOCK_VECTOR, r: a program of flow_form_block_vector for component r.
 * A further program of a block or component is added to its plane entry by
 * entry, in the order of the list.  ONE gather launch then sums everything:
 * lanes [0, nnz) write vals + p*plane_stride, p = 0..3, over cptr / csrc,
 * lanes [nnz, nnz + n) write b[r*n + i] over vptr / vsrc, each sum in the
 * order and arithmetic of the gather of flow_form_block_matrix /
 * flow_form_block_vector: the bits those give for the same programs.  A
 * block or component without a program is set to zero.  No atomics: two calls
 * give the same bits.  Not on strips.
 * scratch (nscratch doubles, checked): nloc^2 * nc per block with a program,
 * + nloc * nc per component with one, + one more plane (nloc^2 * nc, or nloc *
 * nc where only a component does) where a block or component has several. */
#define FLOW_BLOCK_NEWTON 0
#define FLOW_BLOCK_MATRIX 1
#define FLOW_BLOCK_VECTOR 2
int flow_form_block_newton(const flow_mesh* mesh, const flow_space* V, int nprog,
                           const flow_form* forms, const int* kinds,
                           const int* tags, double* scratch, size_t nscratch,
                           double* vals, size_t plane_stride, double* b,
                           void* stream);

/* ---- point evaluation (flow_amd/fem/points.py): u(x), Probes ---------------
 * A uniform bucket grid over the mesh's bounding box, built on the host once
 * per mesh: bucket (ix, iy) = (floor((x - x0) * hx_inv), floor((y - y0) *
 * hy_inv)) clamped to [0, nx-1] x [0, ny-1], id iy*nx + ix; its candidate
 * cells are cells[start[b] .. start[b+1]), every cell whose (padded)
 * bounding box overlaps the bucket, in ascending cell index. */
typedef struct {
  int nx, ny;              /* buckets per axis */
  double x0, y0;           /* lower-left corner of the grid */
  double hx_inv, hy_inv;   /* 1 / bucket width, 1 / bucket height */
  const int* start;        /* nx*ny + 1 */
  const int* cells;        /* start[nx*ny] candidate cells */
} flow_point_grid;

/* Point location, one lane per point.  xy: (2, n) SoA fp64.  Point i belongs
 * to the LOWEST-index cell c whose barycentric coordinates all satisfy
 * lambda_k >= -1e-12, or to none: cell[i] = c or -1 (int32), bary[k*n + i] =
 * lambda_k on that cell ((3, n) fp64; NaN for -1).  The grid only narrows the
 * candidates; the answer does not depend on it, nor on the order or number of
 * the points.  n == 0: nothing launched. */
int flow_locate_points(const flow_mesh* mesh, const flow_point_grid* grid, int n,
                       const double* xy, int* cell, double* bary, void* stream);

/* The form's program at located points, one lane per point: out[o*n + i] =
 * output o (< form->nout) at barycentric bary[., i] of cell[i]; NaN where
 * cell[i] == -1.  The rule and tables are unused; programs holding expr or
 * normal are refused.  Not on strips.  n == 0: nothing launched. */
int flow_form_points(const flow_mesh* mesh, const flow_form* form, int n,
                     const int* cell, const double* bary, double* out,
                     void* stream);

/* Tracer particles (flow_amd/fem/tracers.py): `steps` substeps of size dt of
 * an explicit Runge-Kutta scheme for dx/dt = u(x, t), one lane per particle,
 * one launch.  W: the scalar space of the velocity's components (deg 1 | 2,
 * cell_dofs read); u, u_next: 2 * W->n doubles, component-major; u_next NULL:
 * the field is frozen, else the velocity at fraction theta in [0, 1] of the
 * call's time steps * dt is (1 - theta) u + theta u_next, at each stage's own
 * time.  xy (2, n), cell (n,), bary (3, n): the state in the layout of
 * flow_locate_points, updated in place; on entry cell / bary must be what
 * flow_locate_points gives for xy, and they are again on return.  Every stage
 * point is located by the lowest-index rule.  A substep one of whose stage
 * points, or whose end point, lies in no cell loses the particle: xy keeps
 * the start of that substep, cell = -1, bary = NaN; particles with cell -1
 * are left alone.  dt may be negative.  Two calls give the same bits; steps =
 * k equals k calls of steps = 1 on a frozen field.  Not on strips.  n == 0:
 * nothing launched. */
#define FLOW_ADVECT_EULER 1
#define FLOW_ADVECT_RK2 2      /* midpoint */
#define FLOW_ADVECT_RK4 4      /* classical */
int flow_advect_points(const flow_mesh* mesh, const flow_point_grid* grid,
                       const flow_space* W, const double* u, const double* u_next,
                       int n, double* xy, int* cell, double* bary, double dt,
                       int steps, int scheme, void* stream);

/* ---- field transfer (flow_amd/fem/transfer.py): fem.Transfer -----------------
 * Nearest point of the mesh for points in no cell, one lane per point.  Every
 * point with cell[i] == -1 on entry (what flow_locate_points gives it) gets
 * the nearest point of the mesh's boundary: the boundary facet f with the
 * smallest squared distance to it, ties to the lowest f; cell[i] =
 * facet_cell[f], bary[., i] the barycentric coordinates of the clamped foot
 * point on that cell (the coordinate opposite the facet is exactly 0, all lie
 * in [0, 1]), dist[i] the distance.  Other points keep cell and bary, dist[i]
 * = 0.  facet_grid: the layout of flow_point_grid; its `cells` hold indices
 * into facet_cell / facet_local (nfacets entries: the owning cell and the
 * local facet index of every boundary facet), every facet listed in each
 * bucket its padded bounding box overlaps.  A lane searches the rings of
 * buckets around its own (clamped) bucket outward and stops when no point of
 * a farther ring can be nearer than the best found: the grid narrows the
 * candidates and never changes the answer of the search over all facets.
 * xy: (2, n) SoA; bary: (3, n).  Not on strips.  n == 0: nothing launched. */
int flow_nearest_cells(const flow_mesh* mesh, const flow_point_grid* facet_grid,
                       int nfacets, const int* facet_cell, const int* facet_local,
                       int n, const double* xy, int* cell, double* bary, double* dist,
                       void* stream);

/* out[a*n_to + i] = sum_l phi_l(bary[., i]) u[a*V_from->n + cell_dofs[l][cell[i]]],
 * a < ncomp (1 | 2): the P1 / P2 field u of V_from (deg, n, cell_dofs and vptr
 * read; the cell count is vptr[n] / nloc) at barycentric bary[., i] ((3, n_to)
 * SoA) of its cell cell[i], one lane per target node, all components in one
 * launch.  NaN where cell[i] is no cell.  No atomics: two calls give the same
 * bits.  u and out must differ.  Not on strips.  n_to == 0: nothing launched. */
int flow_transfer_apply(const flow_space* V_from, int ncomp, int n_to,
                        const int* cell, const double* bary, const double* u,
                        double* out, void* stream);

/* ---- conservative transfer (flow_amd/fem/projection.py): fem.Projection -------
 * b[a*V_to->n + i] = int phi_i^to u_a^from dx, a < ncomp (1 | 2): the load
 * vector of the L2 (Galerkin) projection of the P1 / P2 field u of V_from on
 * mesh_from into the P1 / P2 space V_to on mesh_to, integrated exactly over the
 * intersections of the cells of the two meshes.  pptr (mesh_to->nc + 1) / psrc
 * (npairs): per target cell the candidate source cells, ascending -- every
 * source cell that meets the target cell in positive area must be listed,
 * others may be (cells that do not overlap contribute nothing).  One target
 * cell per lane: each listed source triangle is clipped to the target triangle
 * (Sutherland-Hodgman, closed inside test), the polygon fanned from its first
 * vertex and the 7-point degree-5 rule applied to each sub-triangle (exact: the
 * integrand has degree <= 4), all in the order of the list; then
 * scratch[(a*nloc_to + i)*nc_to + c] holds the cell's sums and the gather over
 * V_to->vptr / vsrc adds them into b.  No atomics: two calls give the same
 * bits.  coverage[c] (nc_to doubles, always written) = area of the target cell
 * covered by listed source cells / its area.  scale = 1: the sums of cell c are
 * divided by coverage[c] (the source's mean over the covered part stands for
 * the rest; NaN where coverage is 0), scale = 0: left as they are.
 * u == NULL: the geometry alone -- coverage is filled, V_from, V_to, scratch
 * and b are not read (one launch).
 * NaN in coverage[c] and in the sums of cell c where its row leaves the pair
 * list, names a source cell outside [0, mesh_from->nc) or a dof outside [0,
 * V_from->n); nothing outside the arrays is read.  scratch: ncomp * nloc_to *
 * nc_to doubles.  No alignment beyond that of double is relied on.  u, b,
 * scratch and coverage must differ.  6 * nc < 2^31 on both meshes.  Not on
 * strips. */
int flow_project_load(const flow_mesh* mesh_from, const flow_space* V_from,
                      const flow_mesh* mesh_to, const flow_space* V_to, int ncomp,
                      const int* pptr, const int* psrc, int npairs, const double* u,
                      int scale, double* scratch, double* coverage, double* b,
                      void* stream);

/* ---- norms across meshes (flow_amd/fem/supermesh.py): fem.Supermesh -----------
 * Error norms and inner products of the P1 / P2 field u of V_a on mesh_a and
 * the P1 / P2 field w of V_b on mesh_b (ncomp 1 | 2 components each, component-
 * blocked), integrated exactly over the intersections of the cells of the two
 * meshes, per cell c of mesh_b (the target, as in flow_project_load):
 *   cell_values[c]              = sum_a int_{c ^ mesh_a} (u_a - w_a)^2 dx
 *   cell_values[mesh_b->nc + c] = sum_a int_{c ^ mesh_a} |grad u_a - grad w_a|^2 dx
 * with product = 0, and u_a w_a and grad u_a . grad w_a in their place with
 * product = 1.  Both planes are always written (2 * mesh_b->nc doubles).  pptr /
 * psrc / npairs: the pair list of flow_project_load (cells of mesh_a per cell
 * of mesh_b).  One target cell per lane, the clip, fan and 7-point rule of
 * flow_project_load in the order of the list (the integrands have degree <= 4:
 * exact); nothing is scaled where mesh_a covers a cell in part.
 * totals_host != NULL: totals_host[0], [1] = the sums of the two planes, in a
 * fixed order -- lane t of block b of G = min(ceil(nc / 256), 1024) blocks adds
 * the cells b*256 + t, + 256 G, ... in turn, the block sums its 256 lanes (a
 * shuffle tree per wave of 64, the four waves in turn), one finishing block per
 * plane sums the G partials the same way -- and the call waits for the stream;
 * work: FLOW_REDUCE_WORK doubles.  totals_host == NULL: one launch, no
 * synchronisation, work is not used.  No atomics: two calls give the same bits.
 * NaN in both values of cell c where its row leaves the pair list, names a cell
 * outside [0, mesh_a->nc) or a dof of either space lies outside [0, n); nothing
 * outside the arrays is read.  u and w may be the same buffer; cell_values and
 * work must differ from them and from each other.  6 * nc < 2^31 on both
 * meshes.  Not on strips. */
int flow_supermesh_norms(const flow_mesh* mesh_a, const flow_space* V_a,
                         const flow_mesh* mesh_b, const flow_space* V_b, int ncomp,
                         const int* pptr, const int* psrc, int npairs,
                         const double* u, const double* w, int product,
                         double* cell_values, double* work, double* totals_host,
                         void* stream);

/* ---- adaptive refinement (flow_amd/fem/adapt.py): fem.JumpIndicator ----------
 * eta2[c] = sum over the interior edges E of cell c of
 *     |E| / 24 * int_E sum_{a < ncomp} [grad u_a . n]^2 ds,
 * [.] the jump across E, for the P1 / P2 field u of V (deg, n and cell_dofs
 * read; ncomp 1 | 2, component-blocked); boundary edges contribute nothing.
 * One lane per cell, one launch, no host synchronisation, no atomics: every
 * interior edge is evaluated from both of its cells and two calls give the
 * same bits.  Edge quadrature: the mid point for P1, 2-point Gauss for P2
 * (both exact).  facet_table: 3 * nc ints, entry [i*nc + c] for local facet i
 * (the edge opposite local vertex i) of cell c: -1 on the boundary, else
 * (neighbour << 3) | (the neighbour's local facet << 1) | flip, flip = 0 when
 * the first vertex of the neighbour's facet (facet j: vertices j == 0 ? 1 : 0
 * and j == 2 ? 1 : 2) is the first vertex of this cell's facet, 1 when it is
 * the second.  nc < 2^28.  eta2[c] = NaN where an entry names no cell or no
 * facet, or a dof index lies outside [0, n).  u and eta2 must differ.  Not on
 * strips. */
int flow_jump_indicator(const flow_mesh* mesh, const flow_space* V, int ncomp,
                        const int* facet_table, const double* u, double* eta2,
                        void* stream);

/* ---- recovered gradients (flow_amd/fem/recovery.py): fem.GradientRecovery -----
 * out[(2*a + d)*n + i] = sum_c |T_c| d(u_a)/dx_d|_c(x_i) / sum_c |T_c|, a < ncomp
 * (1 | 2), d = 0, 1, n = V->n: the area-weighted mean, over the cells c of the
 * patch of node i, of the gradient of the P1 / P2 field u of V (component-
 * blocked) in c AT the node (Zienkiewicz-Zhu).  One lane per node, all
 * components in one launch.  The patch of node i is its row vptr[i] ..
 * vptr[i+1] of vsrc; the entry l*nc + c names local node l of cell c (0-2 the
 * vertices, 3-5 the mid points of the edges opposite them) and the terms are
 * added in the order of the map: no atomics, two calls give the same bits, and
 * the planes of one component do not depend on ncomp.  Boundary nodes get the
 * mean over their one-sided patch, nothing else.  NaN at a node whose row is
 * empty or leaves the map, or whose patch names a cell outside [0, nc) or a
 * dof outside [0, n).  V: deg, n, cell_dofs, vptr and vsrc are read.  u and
 * out (2 * ncomp * n doubles) must differ.  6 * nc < 2^31.  Not on strips. */
int flow_recover_gradient(const flow_mesh* mesh, const flow_space* V, int ncomp,
                          const double* u, double* out, void* stream);

/* eta2[c] = sum_{a < ncomp} int_T |G_a - grad u_a|^2 dx, G_a the P_deg vector
 * field with the nodal values G[(2*a + d)*n + i] (the layout
 * flow_recover_gradient writes): the Zienkiewicz-Zhu indicator.  One lane per
 * cell, one launch, no atomics.  rule: nq <= FLOW_FORM_MAX_POINTS rows (xi,
 * eta, w) in device memory, weights summing to 1/2 (flow_form.rule's
 * convention); the integrand has degree 2 * deg.  NaN where a dof index lies
 * outside [0, n).  eta2 must differ from u and G.  Not on strips. */
int flow_zz_indicator(const flow_mesh* mesh, const flow_space* V, int ncomp,
                      const double* u, const double* G, int nq, const double* rule,
                      double* eta2, void* stream);

/* ---- wall distance (flow_amd/fem/distance.py): fem.Distance -------------------
 * nsweeps >= 1 Jacobi sweeps of the monotone Eikonal solver on the P1
 * triangulation of the dofs of V (P1: the cells; P2: every cell cut into its
 * three corner triangles and the middle one, mid points of the straight edges):
 *   new[i] = min(old[i], min over the triangles at i of the Hopf-Lax update of
 *            i from the triangle's two other values),
 * sweep k reading buf_a and writing buf_b for even k and the other way round
 * for odd k (k = 0 .. nsweeps - 1): the result is in buf_b when nsweeps is odd,
 * in buf_a when it is even.  buf_a holds the start: 0 at the sources, +inf
 * elsewhere (or any earlier iterate); an infinite value is never used as an
 * input, and a dof no path of cells connects to a finite value keeps +inf.  One
 * lane per dof walks its row vptr[i] .. vptr[i+1] of vsrc (entry l*nc + c:
 * local node l of cell c); no atomics: two calls give the same bits.  *flag
 * (device memory, zeroed by the caller) is set to 1 by every lane whose value
 * the LAST of the nsweeps sweeps lowered -- a sweep that lowers nothing has
 * reached the fixed point whatever the sweeps before it did.  Nothing is
 * synchronised.  NaN at a dof whose row leaves the map, or whose patch names a
 * cell outside [0, nc) or a dof outside [0, n).  V: deg, n, cell_dofs, vptr and
 * vsrc are read.  buf_a and buf_b (n doubles each) must differ.  6 * nc < 2^31.
 * Not on strips. */
int flow_distance_sweeps(const flow_mesh* mesh, const flow_space* V, int nsweeps,
                         double* buf_a, double* buf_b, int* flag, void* stream);

/* ---- contour lines and level-set measures (flow_amd/fem/isolines.py):
 * fem.Isolines ---------------------------------------------------------------
 * f_h is the continuous piecewise-linear interpolant of the nodal values f (n
 * doubles) of V: the field itself on P1; on P2 every cell is cut into its
 * three corner triangles and the middle one, as for the wall distance, in that
 * order.  A node is above iff f >= c.  A sub-triangle with three finite values
 * that are not all on one side holds one segment of {f_h == c}, between the
 * crossings of two of its sub-edges -- except where the ONE node above lies
 * exactly on c (both crossings are that node: nothing is emitted).  The
 * crossing of the sub-edge with dofs a < b is x_a + t (x_b - x_a),
 * t = (c - f_a) / (f_b - f_a), from the lower dof to the higher whichever cell
 * computes it: the same bits from both cells at an edge.  A segment has the
 * above side on its left.  A sub-triangle with a non-finite value holds no
 * segment and adds nothing to a length or an area.
 *
 * The levels of a launch travel in the kernel arguments (levels: HOST memory,
 * passed on by value; nothing is uploaded): at most
 * FLOW_ISOLINE_LEVELS_PER_LAUNCH of them, level k of the launch being level
 * base + k of the caller's list.  levels->n == 0: nothing is launched.  One
 * lane per cell in all three; no atomics; nothing is synchronised.  V: deg, n
 * and cell_dofs are read.  6 * nc < 2^31.  Not on strips. */
#define FLOW_ISOLINE_LEVELS_PER_LAUNCH 32
typedef struct flow_isoline_levels {
  int n;                                      /* levels in use, 0..32 */
  int base;                                   /* index of the first one */
  double c[FLOW_ISOLINE_LEVELS_PER_LAUNCH];
} flow_isoline_levels;

/* count[cell] (nc ints) = the segments of the cell over the launch's levels.
 * mesh->xy is not read.  A cell that names a dof outside [0, n) counts 1 (the
 * record flow_isoline_emit fills with NaN and -1) and reads nothing outside
 * the arrays. */
int flow_isoline_count(const flow_mesh* mesh, const flow_space* V, const double* f,
                       const flow_isoline_levels* levels, int* count, void* stream);

/* The segments of the launch's levels: cell c writes its count[c] segments at
 * offset[c], offset[c] + 1, ..., ordered by level, then by sub-triangle; count
 * is what flow_isoline_count gave for the same f and levels, offset (nc ints)
 * the caller's exclusive scan of it (plus whatever earlier launches put in
 * front of the cell).  Per segment s: xy[4 s ..] = x0, y0, x1, y1; level[s] =
 * base + k; cell[s]; keys[4 s ..] = a0, b0, a1, b1, the dofs a < b of the two
 * crossed sub-edges; bary[6 s ..] = the barycentric coordinates of both end
 * points in the parent cell.  A record at or past `capacity` is not written,
 * nor one beyond count[c]; a negative offset writes nothing.  A cell that names
 * a dof outside [0, n) writes NaN (xy, bary), -1 (level, keys) and its index
 * (cell) into its one record.  capacity == 0: nothing is launched. */
int flow_isoline_emit(const flow_mesh* mesh, const flow_space* V, const double* f,
                      const flow_isoline_levels* levels, const int* count,
                      const int* offset, int capacity, double* xy, int* level,
                      int* cell, int* keys, double* bary, void* stream);

/* out[2 k] = the length of {f_h == c_k}, out[2 k + 1] = the area of
 * {f_h >= c_k}, k < levels->n, in DEVICE memory (2 * 32 doubles are enough).
 * Every sub-triangle is clipped exactly.  Per level each block of 256 cells
 * adds its lanes in a fixed shape and writes partials[(2 k + q) * nblocks +
 * block], nblocks = (nc + 255) / 256; a second launch adds each row in a
 * fixed order: the grid depends on nc alone and two calls give the same bits.
 * partials: 2 * levels->n * nblocks doubles.  A cell that names a dof outside
 * [0, n) adds nothing. */
int flow_isoline_measure(const flow_mesh* mesh, const flow_space* V, const double* f,
                         const flow_isoline_levels* levels, double* partials,
                         double* out, void* stream);

/* ---- connected components of a level set (flow_amd/fem/regions.py):
 * fem.Regions ----------------------------------------------------------------
 * The graph is the P1 triangulation of the dofs of V, as for the wall distance
 * and the contour lines: on P1 the cells, on P2 every cell cut into its three
 * corner triangles and the middle one, in that order.  A dof is INSIDE iff its
 * value is finite and f >= level (side 0) or f < level (side 1).  Two inside
 * dofs joined by a sub-edge are in one component; its label is its smallest
 * dof.  No atomics anywhere; nothing is synchronised.  6 * nc < 2^31 (rows of
 * the map are entries l*nc + c, slots below are s*nc + c < 4 nc).  Not on
 * strips.
 *
 * label[i] (n ints) = inside(i) ? i : -1.  V: n is read. */
int flow_region_init(const flow_space* V, const double* f, double level, int side,
                     int* label, void* stream);

/* nsweeps >= 1 Jacobi sweeps between two label buffers, sweep k reading buf_a
 * and writing buf_b for even k and the other way round for odd k, as
 * flow_distance_sweeps: the result is in buf_b when nsweeps is odd.  One lane
 * per dof walks its row vptr[i] .. vptr[i+1] of vsrc; for an inside dof
 *   m = min(old[i], min over the inside sub-edge neighbours j of old[j]),
 *   new[i] = old[m]   (one pointer jump),
 * an outside dof (label < 0) stays -1.  A label is always the index of an
 * inside dof of the same component and <= i, so old[m] is a legal read; the
 * fixed point (labels constant on components, L[r] = r) is unique and depends
 * on no ordering.  *flag (device memory, zeroed by the caller) is set to 1 by
 * every lane whose label the LAST of the nsweeps sweeps lowered.  A dof whose
 * row leaves the map, whose patch names a dof outside [0, n) or whose label is
 * no such index is written as -1 and nothing outside the arrays is read.  V:
 * deg, n, cell_dofs, vptr and vsrc are read; mesh->xy is not. */
int flow_region_sweeps(const flow_mesh* mesh, const flow_space* V, int nsweeps,
                       int* buf_a, int* buf_b, int* flag, void* stream);

/* One lane per cell.  ids (n ints): the compact component id of every dof, < 0
 * outside.  Per sub-triangle slot s*nc + cell (s = 0 on P1, 0..3 on P2; nslots
 * = nc or 4 nc): key[slot] = the id of the sub-triangle's inside dofs (they
 * share one) or -1 where it has none or a non-finite value, and
 * vals[r*nslots + slot], r < 3 + ncomp, = the integrals of 1, x, y and g_a
 * over the piece of the sub-triangle where f_h is inside: the whole of it with
 * 3 inside dofs, the corner at the inside node with 1, and with 2 (A, B inside,
 * C outside) the quadrilateral A, B, Q, P, P on A-C and Q on B-C, cut by the
 * diagonal A-Q.  Crossings are those of the contour lines (from the lower dof
 * of the sub-edge).  g (ncomp * G->n doubles, component a at g + a*G->n) is the
 * P1 / P2 polynomial of the parent cell on the space G of the same mesh (deg,
 * n, cell_dofs are read); every triangle is integrated with the edge-midpoint
 * rule, exact for degree 2; areas are absolute values.  Every slot is written,
 * with zeros where there is no piece.  ncomp 0..2; ncomp == 0: G and g are not
 * read.  key == NULL: the keys are not written.  A cell that names a dof
 * outside [0, n) (or of g outside [0, G->n)) writes -1 and zeros. */
int flow_region_moments(const flow_mesh* mesh, const flow_space* V, const double* f,
                        double level, const int* ids, const flow_space* G, int ncomp,
                        const double* g, int* key, double* vals, void* stream);

/* out[r*count + k] = sum over t in [offsets[k], offsets[k+1]) of
 * vals[r*nslots + perm[t]], r < nrows, k < count: one block per (k, r), lanes
 * stride over the segment in a fixed assignment and a block sum of fixed shape
 * finishes -- the same inputs give the same bits.  offsets: count + 1 ints
 * (clipped to [0, nslots]); perm: nslots ints (an entry outside [0, nslots)
 * adds nothing).  count == 0 or nrows == 0: nothing is launched. */
int flow_region_segment_sum(int count, const int* offsets, const int* perm, int nrows,
                            int nslots, const double* vals, double* out, void* stream);

/* The same with the minimum and the maximum: out_min[r*count + k], out_max[..]
 * over vals[r*n + perm[t]]; +inf and -inf for an empty segment. */
int flow_region_segment_minmax(int count, const int* offsets, const int* perm, int nrows,
                               int n, const double* vals, double* out_min,
                               double* out_max, void* stream);

/* ---- reductions of stored fields (flow_amd/fem/snapshots.py): fem.Snapshots ---
 * X is a column-major store of fields: column j starts at X + j*ldx; ldx >= n
 * and even, X (and y) 16-byte aligned, so every column is.
 *
 * out[j] = sum_i X[j*ldx + i] * y[i], j < m (any m >= 1; m == 0 or n == 0:
 * nothing is launched).  out (m doubles) is DEVICE memory: no host
 * synchronisation.  The columns are handled eight per lane around one load of
 * y; the grid is a function of n alone (at most FLOW_MULTI_DOT_BLOCKS blocks),
 * each lane adds its entries in ascending i, the block sum has a fixed shape
 * and a finishing launch adds the block sums in ascending block order: out[j]
 * depends on n, column j and y alone -- the same bits whatever m is and
 * wherever the column sits among the others -- and two calls give the same
 * bits.  No atomics.  work: m * FLOW_MULTI_DOT_BLOCKS doubles.  The caller
 * refuses strips (a rank holds its own rows only): no operand here says so. */
#define FLOW_MULTI_DOT_BLOCKS 1024
int flow_multi_dot(int n, int m, const double* X, size_t ldx, const double* y,
                   double* work, double* out, void* stream);

/* out[k*ldo + i] = (base ? base[i] : 0) + sum_{j < m} C[k*m + j] * X[j*ldx + i],
 * k < r, i < n, the terms added in ascending j (fma): deterministic by
 * construction.  C: r*m doubles in DEVICE memory; base: n doubles or NULL.
 * m >= 1; ldx >= n, ldo >= n (no alignment asked).  One lane per row, eight
 * outputs per lane around one load of X[j][i].  out must not overlap X, base
 * or C (refused).  r == 0 or n == 0: nothing is launched. */
int flow_combine(int n, int m, const double* X, size_t ldx, int r,
                 const double* C, const double* base, double* out, size_t ldo,
                 void* stream);

/* ---- deflation against a nullspace basis (flow_amd/fem/nullspace.py):
 * fem.VectorSpaceBasis ------------------------------------------------------------
 * x <- x - sum_{j < k} Z_j (Z_j^T x) in place, Z_j = Z + j*ldz the columns of a
 * store with the conventions of flow_multi_dot (ldz >= n and even, Z and x
 * 16-byte aligned), 1 <= k <= 8.  Two launches, no temporary, no host
 * synchronisation, no atomics: the first leaves per-block partial sums of all k
 * products around one load of x in work (k * FLOW_MULTI_DOT_BLOCKS doubles) with
 * the lane order, block shape and grid of flow_multi_dot; in the second every
 * block adds the partials of each column in ascending block order and then
 * updates its entries, x[i] = fma(-c_j, Z_j[i], x[i]) for j ascending.  coef (k
 * doubles of DEVICE memory, or NULL) receives c: coef[j] has the bits
 * flow_multi_dot(n, k, Z, ldz, x, ...) leaves in out[j], and x the bits of that
 * call followed by flow_combine(n, k, Z, ldz, 1, -c, x, out, ...).  Neither
 * depends on k or on a column's place among the others beyond their order, and
 * two calls give the same bits.  work, coef, Z and x must not overlap one
 * another (refused, code 2; a refusal launches nothing).  n == 0 or k == 0:
 * nothing is launched.  For a basis that is orthonormal this is the orthogonal
 * projection onto its complement. */
int flow_deflate(int n, int k, const double* Z, size_t ldz, double* x,
                 double* work, double* coef, void* stream);

/* ---- block kernels of the eigensolver (flow_amd/fem/eigen.py): fem.Eigenmodes --
 * X and Y are column-major stores with the conventions above: column j at
 * X + j*ldx, ld >= n and even, the store 16-byte aligned, the padding (entries
 * at and past n of a column) never read or written.
 *
 * Y[:, j] = A X[:, j], j < m, for a scalar operator (kind 0: n = A->n) or a
 * 2x2-block operator (kind 2: n = 2 * A->n in every size check, a column holds
 * component x then component y, A->rowblocks the tiles of the kernels that park
 * two products per nonzero, as for flow_operator_apply); kinds 1, 3 and 4 are
 * refused.  ONE launch: a workgroup loads its CSR-stream tile of A once and
 * runs over the columns in chunks, so the 12 B per nonzero of A (kind 2: the
 * 36 B of the four value planes and the columns) are read once instead of m
 * times.  Column j has exactly the bits flow_operator_apply gives for that
 * column (the same products, the same summation order per row).  No atomics:
 * two calls give the same bits.  Y must not overlap X (refused).  m == 0:
 * nothing is launched.  A refusal (code 2) launches nothing. */
int flow_operator_apply_block(const flow_operator* A, int m, const double* X,
                              size_t ldx, double* Y, size_t ldy, void* stream);
/* The same with the chunk width chosen by the caller (2, 4 or 8 columns; 0: the
 * library's own): for tools/eigen_lab.py.  Kind 2 parks two LDS planes per
 * column (16 KB): 2 or 4 columns, 8 is refused.  The bits do not depend on
 * it. */
int flow_operator_apply_block_chunk(const flow_operator* A, int m, const double* X,
                                    size_t ldx, double* Y, size_t ldy, int mc,
                                    void* stream);

/* out[i*mb + j] = sum_r X[i*ldx + r] * Y[j*ldy + r], i < ma, j < mb: the Gram
 * matrix of two blocks in DEVICE memory (no host synchronisation), one launch
 * plus one finishing launch for all ma*mb entries.  Entry (i, j) has the bits
 * flow_multi_dot(n, ma, X, ldx, Y + j*ldy, ...) leaves in out[i]: it depends on
 * n and its two columns alone, and two calls give the same bits.  No atomics.
 * work: ma * mb * FLOW_MULTI_DOT_BLOCKS doubles.  work and out must not overlap
 * X, Y or each other (refused).  n, ma or mb == 0: nothing is launched. */
int flow_block_gram(int n, int ma, const double* X, size_t ldx, int mb,
                    const double* Y, size_t ldy, double* work, double* out,
                    void* stream);

/* ---- the matrix of a form on a Taylor-Hood space (flow_amd/fem/mixed.py):
 * MixedMatrix ------------------------------------------------------------------
 * A linear operator by blocks over the unknowns velocity x, velocity y,
 * pressure (2 nv + np):
 *   uu     2x2 blocks over the velocity pattern (nv rows): four value planes,
 *          plane 2 r + s = (test component r, trial component s), as the
 *          planes of a kind-2 flow_operator;
 *   up[r]  (test component r, trial p): nv x np, the two planes over ONE
 *          rectangular pattern (space.RectLayout(kv, kp));
 *   pp     np x np over the pressure pattern: one plane;
 *   pu[s]  (test q, trial component s): np x nv, the two planes over ONE
 *          rectangular pattern (space.RectLayout(kp, kv)).
 * Any block may be absent: its value pointer is NULL (the four uu planes are
 * present or absent together); the pattern of an absent block is not read.
 * Value planes and cols as for flow_operator: every plane 16-byte aligned and
 * readable up to index nnz, cols 8-byte aligned and readable at nnz.
 * vtiles (nvtiles + 1) / ptiles (nptiles + 1): row tiles of the velocity and of
 * the pressure rows, each of at most FLOW_SPMV_ROWS_PER_BLOCK consecutive rows
 * holding no more nonzeros than flow_spmv_tile_nnz(kind) in EACH pattern the
 * tile touches: a velocity tile the velocity pattern (kind 2) and the up
 * pattern (kind 0), a pressure tile the pressure pattern and the pu pattern
 * (kind 0).  Built on the host over both row pointers. */
typedef struct {
  int nv, np;              /* dofs of one velocity component, of the pressure */
  int nvtiles, nptiles;
  const int* vrowptr;      /* nv+1 */
  const int* vcols;
  const double* uu[4];
  const int* uprowptr;     /* nv+1 */
  const int* upcols;
  const double* up[2];
  const int* prowptr;      /* np+1 */
  const int* pcols;
  const double* pp;
  const int* purowptr;     /* np+1 */
  const int* pucols;
  const double* pu[2];
  const int* vtiles;       /* nvtiles+1 */
  const int* ptiles;       /* nptiles+1 */
} flow_mixed;

/* y = A x for all blocks in ONE launch of nvtiles + nptiles workgroups; x and
 * y hold 2 nv + np doubles.  A velocity tile does the uu product of both
 * components and then the two up planes (columns and x_p loaded once), a
 * pressure tile the pp row sum and then the two pu planes (columns loaded
 * once); y_u = s_uu + s_up per component, y_p = (s_pp + s_pu0) + s_pu1, a row
 * sum being the products of the row added in ascending k.  Every entry of y
 * has the bits that one flow_operator_apply per block, the results added in
 * that order by flow_axpby(1, t, 1, y), leaves there, for every subset of
 * present blocks (rows that no present block touches: 0.0).  No atomics: two
 * calls give the same bits.  Only a tile's own columns are dereferenced.  y
 * overlapping x is refused (code 2); a refusal launches nothing. */
int flow_mixed_apply(const flow_mixed* A, const double* x, double* y,
                     void* stream);

/* The first half of the block upper triangular preconditioner [[F, up], [0,
 * diag(s)]] in ONE launch over the tiles of flow_mixed_apply: r holds 2 nv + np
 * doubles, sinv (np) the inverse of the pressure diagonal;
 *   z_p[i]        = r_p[i] * sinv[i]                            (np doubles)
 *   ru[c nv + i]  = r[c nv + i] - sum_k up[c][k] (r_p[col_k] * sinv[col_k])
 * for both components (2 nv doubles).  Only the up planes and their pattern
 * are read; an absent plane leaves its component of ru equal to r's.  A
 * velocity tile forms the gathered operand itself, one rounded multiply, and
 * reads no entry of z_p.  Every entry has the bits of the composed sequence
 * flow_vmul(1, r_p, sinv, z_p), a copy of r_u, and per plane
 * flow_operator_apply(up[c], z_p, t) and flow_axpby(-1, t, 1, ru_c).  No
 * atomics: two calls give the same bits.  ru or z_p overlapping r, sinv or
 * each other is refused (code 2); a refusal launches nothing. */
int flow_mixed_upper_rhs(const flow_mixed* A, const double* sinv,
                         const double* r, double* z_p, double* ru,
                         void* stream);

/* ---- running time statistics of a field (flow_amd/fem/statistics.py):
 * fem.Statistics ---------------------------------------------------------------
 * A store of planes of ld doubles each (ld >= n and even, the store 16-byte
 * aligned), in this order: mean[dim]; M2[dim == 1 ? 1 : 3] (00; or 00, 01, 11)
 * where flags & FLOW_STATS_COVARIANCE; per frequency k A_k[dim], B_k[dim];
 * min[dim], max[dim], tmin[dim], tmax[dim] where flags & FLOW_STATS_EXTREMA.
 * Entries at and past n of a plane (the padding) are never read or written.
 *
 * One sample x (dim * n doubles, component a at x + a*n; 8-byte aligned is
 * enough) of weight w at time t, with the host scalars r = w / (W + w) and
 * s = w * W / (W + w), W the weight so far, and freq->c[k] = w cos phi_k,
 * freq->s[k] = -w sin phi_k, phi_k = 2 pi fmod(f_k t, 1) (freq: HOST memory,
 * passed on by value; NULL: no frequencies):
 *   delta_a = x_a - mean_a;  mean_a = fma(r, delta_a, mean_a)
 *   M2_ab = fma(s * delta_a, delta_b, M2_ab)
 *   A_k,a = fma(c[k], x_a, A_k,a);  B_k,a = fma(s[k], x_a, B_k,a)
 *   if x_a < min_a: min_a = x_a, tmin_a = t   (strict; likewise max)
 * ONE launch, one lane per pair of dofs, no LDS, no atomics, no reduction: two
 * identical sequences of calls give the same bits.  Nothing is uploaded or
 * synchronised.  n == 0: nothing is launched.  x must not overlap the planes
 * (refused).  8 n dim + 16 n * planes bytes. */
#define FLOW_STATS_MAX_FREQ 8
#define FLOW_STATS_COVARIANCE 1
#define FLOW_STATS_EXTREMA 2
typedef struct flow_stats_freq {
  int n;                              /* frequencies in use, 0..8 */
  double c[FLOW_STATS_MAX_FREQ];      /*  w cos phi_k */
  double s[FLOW_STATS_MAX_FREQ];      /* -w sin phi_k */
} flow_stats_freq;
int flow_stats_update(int n, int dim, int flags, const flow_stats_freq* freq,
                      double r, double s, double t, const double* x,
                      double* planes, size_t ld, void* stream);

/* Chan's combination of two such stores (same n, dim, flags, nfreq, ld) into
 * `planes`, with the host scalars q = Wb / W and g = Wa Wb / W, W = Wa + Wb:
 *   d_a = mean_b - mean_a;  mean_a = fma(q, d_a, mean_a)
 *   M2_ab = fma(g * d_a, d_b, M2a_ab + M2b_ab);  A, B add
 *   if min_b < min_a: min_a = min_b, tmin_a = tmin_b  (ties keep `planes`')
 * The same lanes as flow_stats_update; the stores must not overlap. */
int flow_stats_merge(int n, int dim, int flags, int nfreq, double q, double g,
                     double* planes, const double* other, size_t ld,
                     void* stream);

/* ---- K7: Dirichlet conditions (bcs= in solve, pressure_correction.py:226,
 * 327,452; bc.apply(A, b), heat.py:113-114).  dofs sorted, in operator
 * numbering (a*n + i). ------------------------------------------------------ */
/* Newton form: rows -> identity (all planes), F[d] = u[d] - g[d]. */
int flow_bc_identity_rows(const flow_operator* A, double* vals_planes,
                          const int* diag_idx, int nbc, const int* dofs,
                          void* stream);
int flow_bc_residual(int nbc, const int* dofs, const double* g, const double* u,
                     double* F, void* stream);
int flow_bc_set_values(int nbc, const int* dofs, const double* g, double* x,
                       void* stream);
/* symmetric elimination (assemble_system semantics, 'symmetric': True):
 * vals_out = vals_in with rows AND columns of marked dofs replaced by identity;
 * isbc: byte mask of length n for the plane's component. */
int flow_bc_symmetric_matrix(int n, const int* rowptr, const int* cols,
                             const double* vals_in, const unsigned char* isbc,
                             double* vals_out, void* stream);
/* out[e] = (a[e] + b[perm[e]]) / 2, e < n: the symmetric part of the value
 * plane a of a block, b (nb entries) being the plane of the transposed block
 * and perm[e] the position in b of the mirror image of entry e (device int32,
 * built once per pattern on the host).  The sum commutes: calling it for (a,
 * b, perm) and for (b, a, inverse perm) gives mirrored entries the same bits.
 * out overlaps neither input; perm[e] outside [0, nb) gives NaN. */
int flow_plane_symmetric_part(int n, const double* a, const double* b, int nb,
                              const int* perm, double* out, void* stream);
/* The same elimination for the four planes of a kind-2 operator (2x2 blocks
 * over one scalar pattern; plane p = 2 r + s at vals + p*stride, stride >= nnz)
 * in one launch: entry (i, j) of plane (r, s) becomes (r == s && i == j) ? 1 : 0
 * where isbc[r*n + i] || isbc[s*n + j], and is copied otherwise.  isbc: 2n
 * bytes in operator numbering.  vals_in and vals_out are distinct buffers. */
int flow_bc_symmetric_blocks(int n, int nnz, const int* rowptr, const int* cols,
                             const double* vals_in, size_t in_stride,
                             const unsigned char* isbc, double* vals_out,
                             size_t out_stride, void* stream);

/* ---- K13/K14: heat operator (heat.py:20-89) and SUPG tau
 * (stabilization.py:50-143) -------------------------------------------------
 * A = matrix of  -kappa/(rho cp) (grad u, grad v) - (conv . grad u, v)
 *     [+ SUPG terms], Msupg = (u, tau conv . grad v) (added to the lumped M).
 * Q: temperature space (deg 1|2), W: scalar space of `conv` (2 comps).
 * tau_out (3*nc, optional): tau at the three vertices of every cell.
 * status_dev: int, set to 1 on device if any tau > 1e3 (the reference throws).
 * scratch: 2*nloc^2*nc. */
int flow_assemble_heat(const flow_mesh* mesh, const flow_space* Q,
                       const flow_space* W, const double* conv, double kappa,
                       double rho_cp, int supg, double* scratch, double* Avals,
                       double* Msupg_vals, double* tau_out, int* status_dev,
                       void* stream);

/* tau alone, one cell per lane: tau (3*nc) at the three vertices of every
 * cell -- the P1 cell lattice an `expr` operand of a form reads -- with the
 * arithmetic of flow_assemble_heat's tau_out; p: the degree of the space tau
 * stabilises (1|2).  No scratch, no matrix.  status_dev as above. */
int flow_supg_tau(const flow_mesh* mesh, const flow_space* W, const double* conv,
                  double kappa, int p, double* tau, int* status_dev, void* stream);

/* SUPG part of the heat load vector with a non-zero source (heat.py:79-86:
 * the `source / rho_cp` term of R2 times tau conv.grad(v)):
 *   b_i = int (source / rho_cp) tau (conv . grad v_i);
 * source: a scalar P0/P1/P2 interpolant per cell (nl = 1, 3, 6; G unused).
 * scratch: nloc*nc. */
int flow_assemble_heat_supg_source(const flow_mesh* mesh, const flow_space* Q,
                                   const flow_space* W, const double* conv,
                                   double kappa, double rho_cp,
                                   const flow_coef* source, double* scratch,
                                   double* b, int* status_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FLOW_HIP_H */
