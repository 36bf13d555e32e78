# -*- coding: utf-8 -*-
'''
Textbook Krylov solvers in extended precision (numpy.longdouble, 64-bit
mantissa), for tests/test_krylov_trajectories_host.py and
tests/test_krylov_trajectories_gpu.py: Hestenes-Stiefel PCG, right-
preconditioned BiCGStab (van der Vorst 1992, rhat = r0) and right-
preconditioned GMRES(m) with modified Gram-Schmidt and Givens rotations,
restarted from the true residual.  In exact arithmetic iterate k of each is
unique, whatever the formulation (Chronopoulos-Gear, one-pass Gram-Schmidt),
so flow_cg_solve / flow_bicgstab_solve / flow_gmres_solve with maxit = k must
leave THESE iterates in x, and report these norms:

  CG        |B r_k|, r_k the recurrence residual (cg_scalar_kernel: "the
            stopping test ... in the PRECONDITIONED norm", S[kRes2] = z.z)
  BiCGStab  |r_k|, the recurrence residual (bicg_scalar_kernel mode 3)
  GMRES     the true |b - A x_k| of an unconverged solve (gmres(): "resid =
            state[kBeta]" behind gmres_begin_kernel); the least-squares
            estimate where a solve with verify = 0 stops on it

and the driver's rules for GMRES: a start with |b - A x0| > |b| is replaced
by zero (gmres_begin_kernel, gmres_drop_start_kernel), x_is_zero skips the
first product, iterate k > m is what floor(k / m) full cycles and one of
k mod m columns leave.

The preconditioners are explicit linear maps built from the host data the
product uploads: Jacobi (the uploaded reciprocal diagonal), the two-level map
D^-1 + P Ainv P^T and the textbook V(1,1) cycle (coarsest inverse as uploaded,
rounded to fp32), and the dense (LU)^-1 of the textbook IKJ ILU(0) of the
colour-permuted matrix in the original numbering.

The tolerance of a device comparison is never taken from device output: the
same textbook algorithm runs in plain fp64 numpy, d = the largest relative
difference to the extended run over the compared iterates (iterates and
reported norms), and

    tol = 100 * max(d, 2^-53 sqrt(N))

-- two decimal digits for the larger constants of the device's pipelined
recurrences, one-pass Gram-Schmidt and blocked sums.  A case compares iterates
0 .. K only while the reference's reported norm stays >= 1e-8 of its first.
Measured with matrices assembled on the host (oracle/fem_oracle.py; the GPU
module measures again on the matrices it reads back from the device, which
differ from these in the last digits):

  case                                      N     K         d       tol
  bicgstab-big-jacobi-zero             263169     8  2.26e-15  5.70e-12
  bicgstab-block-jacobi-zero             1682    12  9.59e-14  9.59e-12
  bicgstab-block-none-nonzero            1682    12  1.19e-13  1.19e-11
  bicgstab-m25-jacobi-zero                 25     8  9.01e-14  9.01e-12
  bicgstab-p2-jacobi-nonzero              841    12  2.58e-14  2.58e-12
  bicgstab-p2-none-zero                   841    12  2.27e-14  2.27e-12
  cg-big-jacobi-zero                   263169     8  5.14e-16  5.70e-12
  cg-m25-jacobi-nonzero                    25    12  5.31e-15  5.31e-13
  cg-m25-none-zero                         25    12  6.96e-16  6.96e-14
  cg-masked-jacobi-nonzero               1682    12  6.68e-16  4.55e-13
  cg-p2-jacobi-kept-g1                    841    12  1.04e-15  3.22e-13
  cg-p2-jacobi-nonzero                    841    12  1.32e-15  3.22e-13
  cg-p2-jacobi-zero                       841    12  1.33e-15  3.22e-13
  cg-p2-none-zero                         841    12  1.17e-15  3.22e-13
  cg-p2-two_level-nonzero                 841    12  1.74e-15  3.22e-13
  cg-p2-two_level-zero                    841    12  2.69e-15  3.22e-13
  cg-planes-jacobi-nonzero               1682    12  1.14e-15  4.55e-13
  cg-planes-jacobi-zero                  1682    12  1.15e-15  4.55e-13
  gmres-big-jacobi-kept-r4             263169    10  3.75e-14  5.70e-12
  gmres-big-jacobi-zero-r4-x1          263169    10  2.52e-14  5.70e-12
  gmres-block-jacobi-dropped-r4          1682    10  6.77e-16  4.55e-13
  gmres-block-jacobi-kept-r4             1682    10  5.10e-16  4.55e-13
  gmres-block-jacobi-zero-r30-v0         1682    12  7.61e-16  4.55e-13
  gmres-block-jacobi-zero-r4             1682    10  6.77e-16  4.55e-13
  gmres-block-none-kept-r7               1682    16  2.00e-15  4.55e-13
  gmres-block-none-zero-r30-x1           1682    16  4.27e-15  4.55e-13
  gmres-m25-jacobi-zero-r30-x1             25     8  6.27e-13  6.27e-11
  gmres-p2-jacobi-kept-r30                841    12  3.82e-15  3.82e-13
  gmres-p2-none-zero-r7-x1                841    16  1.71e-15  3.22e-13
  cg-m25-jacobi-zero-bb_gap                25  k*=3  4.54e-15  4.54e-13
  bicgstab-m25-jacobi-zero-bb_gap          25  k*=2  1.33e-15  1.33e-13
  gmres-m25-jacobi-zero-bb_gap-r30         25  k*=3  3.47e-13  3.47e-11

and the cases whose preconditioners need the library to build, measured the
same way (host, reference against reference) by the GPU module's fixture:

  cg-p2-mg-zero / cg-p2-mg_levels-zero    841    12  1.94e-14  1.94e-12
  cg-p2-mg-nonzero                        841    12  3.97e-15  3.97e-13
  bicgstab-p2-ilu-zero                    841    12  3.70e-13  3.70e-11
  bicgstab-block-ilu-zero                1682    12  2.84e-13  2.84e-11
  bicgstab-block-ilu-nonzero             1682    12  6.42e-13  6.42e-11
  gmres-p2-ilu-zero-r30                   841    12  2.51e-13  2.51e-11
  gmres-block-ilu-zero-r30-x1            1682    12  5.55e-14  5.55e-12
  gmres-block-ilu-kept-r30-v0            1682    12  4.64e-14  4.64e-12

Mutants of the reference (`mutant=`), the largest departure from the true
reference over the compared iterates of the case named, as a multiple of that
case's tolerance (the host test asserts >= 1000):

  mutant             case                           tolerances
  drop_h4            gmres-block-none-zero-r30-x1    1.91e+11
  drop_h4            gmres-p2-none-zero-r7-x1        2.86e+11
  estimated_restart  gmres-block-jacobi-zero-r4      4.58e+12
  estimated_restart  gmres-p2-none-zero-r7-x1        2.13e+13
  half_coarse        cg-p2-two_level-zero            1.29e+12
  half_coarse        cg-p2-two_level-nonzero         1.29e+12
  left:bicgstab      bicgstab-block-jacobi-zero      2.31e+12
  left:bicgstab      bicgstab-p2-jacobi-nonzero      8.65e+12
  left:gmres         gmres-block-jacobi-zero-r4      4.86e+13
  left:gmres         gmres-p2-jacobi-kept-r30        5.75e+13
  shift:bicgstab     bicgstab-block-jacobi-zero      1.03e+14
  shift:cg           cg-p2-jacobi-zero               2.17e+15
  shift:gmres        gmres-block-jacobi-zero-r4      1.55e+15
  stale_beta         cg-p2-jacobi-zero               3.87e+12
  stale_beta         cg-m25-none-zero                1.05e+15
'''
import numpy
import scipy.sparse as sp

EXT = numpy.longdouble
assert numpy.finfo(EXT).nmant >= 63, 'numpy.longdouble is not extended here'

FLOOR = 1.0e-8        # compared while norm_k / norm_0 >= FLOOR
MARGIN = 100.0
MIN_ITERATES = 6


def norm(v):
    return numpy.sqrt(v.dot(v))


class Csr(object):
    '''y = A x by hand (numpy.add.reduceat) in `dtype`; empty rows give 0.'''

    def __init__(self, A, dtype):
        A = sp.csr_matrix(A)
        self.shape = A.shape
        self.rp = A.indptr.astype(numpy.int64)
        self.ci = A.indices.astype(numpy.int64)
        self.v = A.data.astype(dtype)
        self.rows = numpy.nonzero(numpy.diff(self.rp))[0]
        self.dtype = dtype

    def __call__(self, x):
        y = numpy.zeros(self.shape[0], dtype=self.dtype)
        if len(self.rows):
            y[self.rows] = numpy.add.reduceat(self.v * x[self.ci],
                                              self.rp[self.rows])
        return y


class Dense(object):
    def __init__(self, A, dtype):
        self.A = numpy.asarray(A).astype(dtype)

    def __call__(self, x):
        return self.A.dot(x)


# -- the preconditioners as explicit maps --------------------------------------
def identity(dtype=EXT):
    return lambda r: r.copy()


def jacobi(dinv, dtype=EXT):
    '''dinv: the fp64 reciprocal diagonal as uploaded.'''
    d = numpy.asarray(dinv).astype(dtype)
    return lambda r: d * r


def two_level(dinv, agg_of, Ainv32, dtype=EXT, weight=1.0):
    '''D^-1 + weight P Ainv P^T, P the piecewise-constant prolongation of
    agg_of (-1: left out), Ainv32 the fp32 array as uploaded (nc x lda).'''
    d = numpy.asarray(dinv).astype(dtype)
    agg_of = numpy.asarray(agg_of, dtype=numpy.int64)
    free = numpy.nonzero(agg_of >= 0)[0]
    nc = int(agg_of.max()) + 1
    assert Ainv32.dtype == numpy.float32
    Ai = Ainv32[:nc, :nc].astype(dtype) * dtype(weight)

    def B(r):
        rc = numpy.zeros(nc, dtype=dtype)
        numpy.add.at(rc, agg_of[free], r[free])
        z = d * r
        z[free] += Ai.dot(rc)[agg_of[free]]
        return z
    return B


def vcycle(host_levels, Ainv32, omega, dtype=EXT):
    '''The textbook V(1,1) cycle of Multigrid(..., keep_host=True).host_levels
    = [(A_l, D_l, P_l)], damped Jacobi omega, the coarsest inverse rounded to
    fp32 as uploaded.'''
    lv = [(Csr(A, dtype), numpy.asarray(D).astype(dtype), Csr(P, dtype),
           Csr(P.T.tocsr(), dtype)) for A, D, P in host_levels]
    nc = host_levels[-1][2].shape[1]
    assert Ainv32.dtype == numpy.float32
    Ai = Ainv32[:nc, :nc].astype(dtype)
    w = dtype(omega)

    def cycle(l, r):
        if l == len(lv):
            return Ai.dot(r)
        A, D, P, PT = lv[l]
        x = w * r / D
        x = x + P(cycle(l + 1, PT(r - A(x))))
        return x + w * (r - A(x)) / D
    return lambda r: cycle(0, r)


def ilu0_inverse(blocks, old_of_new):
    '''Dense blockdiag((LU)^-1) in the original numbering: LU the textbook
    IKJ ILU(0) (tests/test_hip_ilu.py) of each block permuted by old_of_new.
    fp64 triangular inverses (unit lower L, U), exact to their conditioning.'''
    import scipy.linalg as sla
    from test_hip_ilu import _ilu0_reference
    perm = numpy.asarray(old_of_new, dtype=numpy.int64)
    n = len(perm)
    out = numpy.zeros((len(blocks) * n, len(blocks) * n))
    P = sp.csr_matrix((numpy.ones(n), (numpy.arange(n), perm)), shape=(n, n))
    for k, A in enumerate(blocks):
        Ap = (P @ sp.csr_matrix(A) @ P.T).tocsr()
        Ap.sort_indices()
        LU, _ = _ilu0_reference(Ap)
        L = (sp.tril(LU, -1) + sp.identity(n)).toarray()
        U = sp.triu(LU).toarray()
        eye = numpy.eye(n)
        inv = sla.solve_triangular(
            U, sla.solve_triangular(L, eye, lower=True, unit_diagonal=True),
            lower=False)
        idx = k * n + perm
        out[numpy.ix_(idx, idx)] = inv
    return out


# -- the solvers --------------------------------------------------------------------
class Trajectory(object):
    '''xs[k], norms[k] (what the device reports for iterate k), bnorm (the
    norm of b the stopping test divides by); GMRES: est[k], the least-squares
    estimate.'''

    def __init__(self, xs, norms, bnorm, est=None):
        self.xs, self.norms, self.bnorm, self.est = xs, norms, bnorm, est

    def shifted(self):
        '"returns iterate k + 1 for k"'
        return Trajectory(self.xs[1:], self.norms[1:], self.bnorm,
                          self.est[1:] if self.est is not None else None)


def pcg(A, B, b, x0, steps, dtype=EXT, mutant=None):
    '''Hestenes-Stiefel PCG.  mutant 'stale_beta': beta from the previous
    gamma (one iteration stale).'''
    b = numpy.asarray(b).astype(dtype)
    x = numpy.asarray(x0).astype(dtype)
    r = b - A(x)
    z = B(r)
    p = z.copy()
    gamma = r.dot(z)
    xs, norms = [x.copy()], [norm(z)]
    stale = dtype(0.0)
    for _ in range(steps):
        q = A(p)
        alpha = gamma / p.dot(q)
        x = x + alpha * p
        r = r - alpha * q
        z = B(r)
        gnew = r.dot(z)
        beta = gnew / gamma
        p = z + (stale if mutant == 'stale_beta' else beta) * p
        stale, gamma = beta, gnew
        xs.append(x.copy())
        norms.append(norm(z))
    return Trajectory(xs, norms, norm(B(b)))


def bicgstab(A, B, b, x0, steps, dtype=EXT, mutant=None):
    '''van der Vorst 1992, right-preconditioned, rhat = r0.  mutant 'left':
    the left-preconditioned system B A x = B b.'''
    b = numpy.asarray(b).astype(dtype)
    if mutant == 'left':
        A0, B0 = A, B
        A, B, b = (lambda v: B0(A0(v))), identity(dtype), B0(b)
    x = numpy.asarray(x0).astype(dtype)
    r = b - A(x)
    rhat = r.copy()
    rho = alpha = omega = dtype(1.0)
    v = numpy.zeros_like(r)
    p = numpy.zeros_like(r)
    xs, norms = [x.copy()], [norm(r)]
    for _ in range(steps):
        rho_new = rhat.dot(r)
        beta = (rho_new / rho) * (alpha / omega)
        p = r + beta * (p - omega * v)
        y = B(p)
        v = A(y)
        alpha = rho_new / rhat.dot(v)
        s = r - alpha * v
        z = B(s)
        t = A(z)
        omega = t.dot(s) / t.dot(t)
        x = x + alpha * y + omega * z
        r = s - omega * t
        rho = rho_new
        xs.append(x.copy())
        norms.append(norm(r))
    return Trajectory(xs, norms, norm(b))


def gmres(A, B, b, x0, steps, m, dtype=EXT, x_is_zero=False, mutant=None):
    '''Right-preconditioned GMRES(m), modified Gram-Schmidt, Givens rotations,
    restarts from the true residual; norms = the true |b - A x_k|.
    mutants: 'left' (B A x = B b), 'drop_h4' (the coefficient against V_4 is
    dropped in step 5 and later of a cycle), 'estimated_restart' (a restart
    continues from the last basis vector scaled with the residual estimate
    instead of from b - A x).'''
    b = numpy.asarray(b).astype(dtype)
    if mutant == 'left':
        A0, B0 = A, B
        A, B, b = (lambda v: B0(A0(v))), identity(dtype), B0(b)
    n = len(b)
    x = numpy.zeros(n, dtype=dtype) if x_is_zero else \
        numpy.asarray(x0).astype(dtype)
    r = b.copy() if x_is_zero else b - A(x)
    if norm(r) > norm(b):             # a start worse than zero is dropped
        x = numpy.zeros(n, dtype=dtype)
        r = b.copy()
    xs, norms, est = [x.copy()], [norm(r)], [norm(r)]
    k = 0
    while k < steps:
        xc = x
        beta = norm(r)
        V, Z = [r / beta], []
        R = numpy.zeros((m + 1, m), dtype=dtype)
        cs = numpy.zeros(m, dtype=dtype)
        sn = numpy.zeros(m, dtype=dtype)
        g = numpy.zeros(m + 1, dtype=dtype)
        g[0] = beta
        for j in range(min(m, steps - k)):
            Z.append(B(V[j]))
            w = A(Z[j])
            for i in range(j + 1):
                if mutant == 'drop_h4' and i == 4 and j >= 5:
                    continue
                R[i, j] = w.dot(V[i])
                w = w - R[i, j] * V[i]
            R[j + 1, j] = norm(w)
            V.append(w / R[j + 1, j])
            for i in range(j):
                t = cs[i] * R[i, j] + sn[i] * R[i + 1, j]
                R[i + 1, j] = -sn[i] * R[i, j] + cs[i] * R[i + 1, j]
                R[i, j] = t
            d = numpy.sqrt(R[j, j]**2 + R[j + 1, j]**2)
            cs[j], sn[j] = R[j, j] / d, R[j + 1, j] / d
            R[j, j], R[j + 1, j] = d, 0.0
            g[j + 1] = -sn[j] * g[j]
            g[j] = cs[j] * g[j]
            y = numpy.zeros(j + 1, dtype=dtype)
            for i in range(j, -1, -1):
                y[i] = (g[i] - R[i, i + 1:j + 1].dot(y[i + 1:])) / R[i, i]
            x = xc.copy()
            for i in range(j + 1):
                x = x + y[i] * Z[i]
            k += 1
            xs.append(x)
            est.append(abs(g[j + 1]))
            norms.append(norm(b - A(x)))
        if mutant == 'estimated_restart':
            r = V[-1] * abs(g[j + 1])
        else:
            r = b - A(x)
    return Trajectory(xs, norms, norm(b), est)


SOLVERS = {'cg': pcg, 'bicgstab': bicgstab, 'gmres': gmres}


# -- systems ----------------------------------------------------------------------
class System(object):
    '''A flow_operator of `kind` over one CSR pattern as host data: planes in
    pattern order (what ops.Matrix takes), the scipy matrix of the whole
    operator (as ops.Matrix.to_scipy builds it) and the fp64 reciprocal
    diagonal.'''

    def __init__(self, kind, rowptr, cols, planes, mask=None, dinv=None):
        self.kind, self.rowptr, self.cols = kind, rowptr, cols
        self.planes = [numpy.asarray(p, dtype=numpy.float64) for p in planes]
        self.mask = mask
        n = len(rowptr) - 1
        self.n = n
        P = [sp.csr_matrix((p, cols, rowptr), shape=(n, n)) for p in self.planes]
        if kind == 0:
            A = P[0]
        elif kind == 1:
            A = sp.block_diag(P, format='csr')
        elif kind == 2:
            A = sp.bmat([[P[0], P[1]], [P[2], P[3]]], format='csr')
        else:
            m = (numpy.asarray(mask) != 0).astype(float)
            A = sp.block_diag(
                [sp.diags(m[c * n:(c + 1) * n]).dot(P[0])
                 + sp.diags(1.0 - m[c * n:(c + 1) * n]) for c in range(2)],
                format='csr')
        self.A = A.tocsr()
        self.N = self.A.shape[0]
        self.dinv = 1.0 / self.A.diagonal() if dinv is None else dinv
        self._ops = {}

    def op(self, dtype):
        if dtype not in self._ops:
            self._ops[dtype] = Csr(self.A, dtype)
        return self._ops[dtype]


def pattern_values(M, rowptr, cols):
    '''The values of a scipy matrix in the order of a CSR pattern.'''
    rows = numpy.repeat(numpy.arange(len(rowptr) - 1), numpy.diff(rowptr))
    return numpy.asarray(sp.csr_matrix(M)[rows, cols]).ravel()


def small_systems(p1, p2):
    '''p1 = (rowptr, cols, M) of P1 on UnitSquareMesh(4, 4); p2 = (rowptr,
    cols, M, K) of P2 on UnitSquareMesh(10, 10, 'crossed'), values in pattern
    order.  dict name -> System (the right-hand sides and starts: starts()).'''
    rng = numpy.random.RandomState(4)
    rp, ci, M, K = p2
    n = len(rp) - 1
    out = {'m25': System(0, p1[0], p1[1], [p1[2]])}
    a = M + 0.01 * K
    out['p2'] = System(0, rp, ci, [a])
    out['planes'] = System(1, rp, ci, [a, M + 0.05 * K])
    # (the perturbed 2x2-block system of test_bicgstab_matches_direct_solve)
    pert = 0.02 * rng.standard_normal((4, len(M))) * abs(M).max()
    zero = numpy.zeros_like(M)
    out['block'] = System(2, rp, ci, [a + pert[0], zero + pert[1],
                                      zero + pert[2], a + pert[3]])
    free = (rng.uniform(size=2 * n) > 0.07).astype(numpy.uint8)
    out['masked'] = System(4, rp, ci, [M], mask=free)
    return out


def starts(name, S):
    '''b and the start vectors of a system: zero, nonzero (arbitrary; masked:
    carrying the boundary values), kept (|b - A x0| < |b|, |B r0| < |B b|),
    dropped (1e3 * noise), and `b_gap` (zero start): three eigenvectors of
    D^-1 A and 1e-4 noise -- the residual of every solver drops by more than
    a factor 10 at iterate 3 (the counts).'''
    import zlib
    rng = numpy.random.RandomState(zlib.crc32(name.encode()) % 2**31)
    N = S.N
    b = rng.standard_normal(N)
    noise = rng.standard_normal(N)
    out = {'zero': numpy.zeros(N), 'nonzero': rng.standard_normal(N)}
    if S.kind == 4:
        g = rng.standard_normal(N)
        fixed = numpy.asarray(S.mask) == 0
        b[fixed] = g[fixed]
        out['nonzero'][fixed] = g[fixed]
        out['zero'] = None            # (not a start that carries the values)
    # half a damped Jacobi step plus noise: keeps every residual norm below
    # that of zero (asserted by the host test and the GPU module)
    out['kept'] = 0.5 * S.dinv * b + 1.0e-3 * noise * abs(S.dinv * b).max()
    out['dropped'] = 1.0e3 * noise
    out['b'] = b
    if N <= 64:
        import scipy.linalg as sla
        lam, vec = sla.eigh(S.A.toarray(), numpy.diag(1.0 / S.dinv))
        v = vec[:, 0] + vec[:, N // 2] + vec[:, -1]
        bg = (v + 1.0e-4 * noise * abs(v).max()) / S.dinv
        out['b_gap'] = bg
    return out


# -- the cases (solver, system, preconditioner, start, options) ---------------------------
# K: iterates compared at most (cut where the reference norm falls below FLOOR)
def _case(solver, system, pre, start, K=12, **kw):
    tag = '-'.join([solver, system, pre, start]
                   + ['%s%s' % (k[0], v) for k, v in sorted(kw.items())])
    return dict(id=tag, solver=solver, system=system, pre=pre, start=start, K=K,
                opts=kw)


CASES = [
    # CG, kind 0
    _case('cg', 'm25', 'none', 'zero'),
    _case('cg', 'm25', 'jacobi', 'nonzero'),
    _case('cg', 'p2', 'none', 'zero'),
    _case('cg', 'p2', 'jacobi', 'zero'),
    _case('cg', 'p2', 'jacobi', 'nonzero'),
    _case('cg', 'p2', 'jacobi', 'kept', guarded=1),
    _case('cg', 'p2', 'two_level', 'zero'),
    _case('cg', 'p2', 'two_level', 'nonzero'),
    _case('cg', 'p2', 'mg', 'zero'),
    _case('cg', 'p2', 'mg', 'nonzero'),
    _case('cg', 'p2', 'mg_levels', 'zero'),
    # kind 1 (two SPD planes), kind 4 (masked rows)
    _case('cg', 'planes', 'jacobi', 'zero'),
    _case('cg', 'planes', 'jacobi', 'nonzero'),
    _case('cg', 'masked', 'jacobi', 'nonzero'),
    _case('cg', 'big', 'jacobi', 'zero', K=8),
    # BiCGStab, kinds 0 and 2
    _case('bicgstab', 'm25', 'jacobi', 'zero'),
    _case('bicgstab', 'p2', 'none', 'zero'),
    _case('bicgstab', 'p2', 'jacobi', 'nonzero'),
    _case('bicgstab', 'p2', 'ilu', 'zero'),
    _case('bicgstab', 'block', 'none', 'nonzero'),
    _case('bicgstab', 'block', 'jacobi', 'zero'),
    _case('bicgstab', 'block', 'ilu', 'zero'),
    _case('bicgstab', 'block', 'ilu', 'nonzero'),
    _case('bicgstab', 'big', 'jacobi', 'zero', K=8),
    # GMRES
    _case('gmres', 'm25', 'jacobi', 'zero', K=8, restart=30, x_is_zero=1),
    _case('gmres', 'p2', 'none', 'zero', K=16, restart=7, x_is_zero=1),
    _case('gmres', 'p2', 'jacobi', 'kept', K=12, restart=30),
    _case('gmres', 'p2', 'ilu', 'zero', restart=30),
    _case('gmres', 'block', 'none', 'zero', K=16, restart=30, x_is_zero=1),
    _case('gmres', 'block', 'jacobi', 'zero', K=12, restart=30, verify=0),
    _case('gmres', 'block', 'jacobi', 'kept', K=10, restart=4),
    _case('gmres', 'block', 'jacobi', 'dropped', K=10, restart=4),
    _case('gmres', 'block', 'jacobi', 'zero', K=10, restart=4),
    _case('gmres', 'block', 'none', 'kept', K=16, restart=7),
    _case('gmres', 'block', 'ilu', 'zero', restart=30, x_is_zero=1),
    _case('gmres', 'block', 'ilu', 'kept', restart=30, verify=0),
    _case('gmres', 'big', 'jacobi', 'zero', K=10, restart=4, x_is_zero=1),
    _case('gmres', 'big', 'jacobi', 'kept', K=10, restart=4),
    ]
# the counts: rtol between the reference's residuals at k* - 1 and k*
COUNT_CASES = [
    _case('cg', 'm25', 'jacobi', 'zero', K=6, b='b_gap'),
    _case('bicgstab', 'm25', 'jacobi', 'zero', K=6, b='b_gap'),
    _case('gmres', 'm25', 'jacobi', 'zero', K=6, b='b_gap', restart=30),
    ]
HOST_PRECONDITIONERS = ('none', 'jacobi', 'two_level')


def reference(case, S, B, vecs, dtype=EXT, mutant=None, steps=None):
    '''The trajectory of a case: S the System, B(dtype) the preconditioner
    map, vecs = starts(...).'''
    opts = case['opts']
    b = vecs[opts.get('b', 'b')]
    x0 = vecs[case['start']]
    kw = {}
    if case['solver'] == 'gmres':
        kw = dict(m=opts['restart'], x_is_zero=bool(opts.get('x_is_zero')))
    steps = case['K'] if steps is None else steps
    shift = mutant == 'shift'
    t = SOLVERS[case['solver']](S.op(dtype), B(dtype), b, x0,
                                steps + (1 if shift else 0), dtype=dtype,
                                mutant=None if shift else mutant, **kw)
    return t.shifted() if shift else t


def compared(t, K):
    '''Iterates 0 .. K' <= K compared: while norms[k] / norms[0] >= FLOOR.'''
    k = 0
    while k + 1 <= K and t.norms[k + 1] >= FLOOR * t.norms[0]:
        k += 1
    return k


def rel(a, ref):
    '''|a - ref| / |ref| in l2 (0 / 0 = 0), in extended precision.'''
    a = numpy.asarray(a).astype(EXT)
    ref = numpy.asarray(ref).astype(EXT)
    d = float(norm(numpy.atleast_1d(a - ref)))
    s = float(norm(numpy.atleast_1d(ref)))
    return d / s if s > 0.0 else d


def rel_max(a, ref):
    a = numpy.asarray(a).astype(EXT)
    ref = numpy.asarray(ref).astype(EXT)
    s = float(abs(ref).max())
    d = float(abs(a - ref).max())
    return d / s if s > 0.0 else d


def departure(t, ref, K):
    '''The largest relative difference between two trajectories over the
    iterates 0 .. K: iterates (l2) and reported norms.'''
    worst = 0.0
    for k in range(K + 1):
        worst = max(worst, rel(t.xs[k], ref.xs[k]),
                    rel(t.norms[k], ref.norms[k]))
    return worst


class Measured(object):
    '''A case measured reference against reference: ext (the trajectory), K
    (iterates compared), d (fp64 textbook run against it), tol.'''

    def __init__(self, case, S, B, vecs):
        self.ext = reference(case, S, B, vecs)
        self.K = compared(self.ext, case['K'])
        self.f64 = reference(case, S, B, vecs, dtype=numpy.float64)
        self.d = departure(self.f64, self.ext, self.K)
        self.floor = 2.0**-53 * numpy.sqrt(S.N)
        self.tol = MARGIN * max(self.d, self.floor)


def count_target(t, solver):
    '''(k*, rtol): the first iterate whose relative residual, in the norm
    the solver tests, lies a factor >= 10 below the one before it; rtol their
    geometric mean.'''
    rels = [float(v / t.bnorm) for v in (t.est if solver == 'gmres' else t.norms)]
    for k in range(1, len(rels)):
        if rels[k - 1] >= 10.0 * rels[k]:
            return k, float(numpy.sqrt(rels[k - 1] * rels[k])), rels
    raise AssertionError('no factor-10 gap in %r' % (rels,))


def count_tolerance(m, kstar):
    '''The tolerance of a count case: measured over the iterates 0 .. k*.'''
    return MARGIN * max(departure(m.f64, m.ext, kstar), m.floor)
