# -*- coding: utf-8 -*-
'''
The smallest eigenpairs of the generalized symmetric problem a(u, v) ==
lambda m(u, v) on the device: Laplace and heat eigenmodes, decay rates,
Poincare and Friedrichs constants -- dolfin's SLEPcEigenSolver, for the case
it is mostly used for.

    E = Eigenmodes(a, m=None, bcs=None)     # rank-2 forms on one scalar P1 / P2
                                            # (or vector: "Vector spaces" below)
    E = Eigenmodes.from_matrices(A, M, isbc=None)     # Matrix objects, kind 0
                                                      # (or both kind 2)
    r = E.solve(k, rtol=1e-8, maxit=200, guard=None, preconditioner='jacobi',
                initial=None, error_on_nonconvergence=True)
    r.values, r.modes, r.residuals, r.iterations, r.converged
    E.rayleigh(u)
    eigensolve(a, m, bcs, k, **kw)          # the one-off spelling

The method is LOBPCG (Knyazev 2001) on a block of b = k + guard columns.  The
basis S = [X, P, W] -- the iterates, the directions of the last step and the
preconditioned residuals -- sits in one column store (column stride ld = N
rounded up to even, as fem.Snapshots keeps its columns), with A S and M S
beside it: 9 b vectors.  flow_combine refuses an output that overlaps its
input, so a second set of the same size takes the rotated block and the two
swap: 18 b + b vectors in all.

One iteration:

    Matrix.apply_block   A W and M W for the new columns: two launches, each
                         streaming its matrix once (csrc/eigen_kernels.hip)
    flow_block_gram      S^T A S, S^T M S, and the squared norms of the
                         residuals and of M X: four calls of two launches
    one read-back        of all of them (the only wait for the device)
    rayleigh_ritz        host numpy / scipy on the (<= 3b)^2 Gram pair
    one upload           of the coefficients
    flow_combine         new X, P and A X, A P, M X, M P out of the stores
                         (3 ceil((b + na) / 8) launches), no new products
    flow_combine         R_j = A x_j - lambda_j M x_j, one launch per column
    preconditioner       W_j = T R_j per active column: flow_vmul with the
                         masked inverse diagonal ('jacobi'), or
                         flow_two_level_apply with an aggregate CoarseSpace
                         ('two_level')

Converged columns are soft-locked: they stay in X and take part in the
Rayleigh-Ritz step, but get no W and no P column (na: the active ones).  A
pair counts as converged when |A x - lambda M x|_2 <= rtol max(|lambda|,
lambda_ref) |M x|_2, lambda_ref the largest of the k current Ritz values (a
zero eigenvalue of a pure Neumann problem has a scale that way).

Dirichlet conditions.  Both matrices go through symmetric_bc_matrix, the start
block is masked to zero on the Dirichlet dofs, and every operation keeps those
entries at zero (identity rows times zero, combinations of zeros, an inverse
diagonal and a coarse space that leave them out): the iteration runs in the
constrained subspace and the unit eigenpairs of the identity rows never enter.

The loop (lobpcg) is written against a backend of block operations -- load,
apply A and M, Gram matrices, rotate, precondition -- with a device backend
and a numpy / scipy one (HostBackend), so the same loop runs without a GPU.

Same call, same bits: the start block comes from a fixed seed, the kernels
have a fixed summation order and the host algebra is deterministic.

Limits.  Symmetric problems only (a form that forms.is_symmetric_table does
not accept is refused unless symmetric=True vouches for it), the smallest
eigenvalues only (no shift-invert), b <= 32, not on strips.  Eigenvectors of
clustered eigenvalues are accurate as a subspace, not one by one: compare
subspaces (principal angles) there.

Vector spaces.  vector_eigenmodes(True) (a process switch like
vector_arguments, which the forms need as well; off: the NotImplementedError
there was) lets a and m live on one P1 / P2 VectorFunctionSpace W: vibration
modes of an elastic body, the vector Laplacian, Korn constants.  Component
views and mixed spaces stay refused.  A and M are then kind-2 matrices (four
value planes over the scalar pattern), every vector has 2N entries,
component-blocked, and the column stride is 2N.  m=None is dot(u, v)*dx.
bcs are conditions on W and on W.sub(i); both matrices go through
symmetric_bc_blocks, and isbc / free have 2N entries in operator numbering.
Matrix.apply_block streams all four planes once per launch (36 B per
nonzero once instead of per column), every column with the bits of
flow_operator_apply.  modes are vector Functions on W; initial takes vector
Functions; rayleigh(u) takes 2N entries.  'jacobi' is the inverse diagonal of
the planes A_xx and A_yy.  'two_level' is component-wise: z = [T_xx r_x ; T_yy
r_y], each T_cc flow_two_level_apply with a CoarseSpace of the plane A_cc of
the eliminated matrix, that component's half of the Dirichlet mask, and
singular= "the component has no Dirichlet dof"; it is block-diagonal and SPD
and ignores the coupling planes A_xy, A_yx.  Limits there: the mass matrix of
dot(u, v)*dx is a kind-2 matrix whose off-diagonal planes are zero and are
streamed all the same (the cost is accepted and not measured); a free body
returns its three rigid-body modes as (numerically) zero eigenvalues;
symmetric problems and the smallest eigenvalues only, k + guard <= 32, not on
strips.
'''
import numpy

from .forms import _Switch

MAX_BLOCK = 32
SEED = 20011


# -- host algebra (numpy / scipy only) --------------------------------------------
def rayleigh_ritz(GA, GM):
    '''The Rayleigh-Ritz step on the Gram pair GA = S^T A S, GM = S^T M S of
    a basis S of s columns: (theta, C) with theta ascending, C^T GM C = I and
    C^T GA C = diag(theta), so that S C are the Ritz vectors.

    Both matrices are symmetrised, and scaled by D = diag(GM)^-1/2 (the
    columns of S may differ by orders of magnitude).  Where the Cholesky
    factor of the scaled GM fails or has a pivot below 1e-7 -- directions of
    S that the others reproduce to rounding, as P and W do near convergence --
    the basis is reduced to the eigenvectors of the scaled GM above s eps
    times the largest: C then has fewer than s columns.'''
    import scipy.linalg
    GA = numpy.asarray(GA, dtype=float)
    GM = numpy.asarray(GM, dtype=float)
    s = GM.shape[0]
    if GA.shape != (s, s) or GM.shape != (s, s) or s < 1:
        raise ValueError('GA, GM: two square matrices of one size')
    GA = 0.5 * (GA + GA.T)
    GM = 0.5 * (GM + GM.T)
    d = numpy.diag(GM).copy()
    if not (numpy.isfinite(GA).all() and numpy.isfinite(GM).all()):
        raise ValueError('GA, GM: not finite')
    live = d > 0.0
    if not live.any():
        raise ValueError('GM: no column of positive norm')
    scale = numpy.zeros(s)
    scale[live] = 1.0 / numpy.sqrt(d[live])
    GAs = GA * scale[:, None] * scale[None, :]
    GMs = GM * scale[:, None] * scale[None, :]
    B = None
    if live.all():
        try:
            L = numpy.linalg.cholesky(GMs)
            if numpy.diag(L).min() >= 1.0e-7:
                # B = L^-T: B^T GMs B = I
                B = scipy.linalg.solve_triangular(
                    L, numpy.eye(s), lower=True).T
        except numpy.linalg.LinAlgError:
            B = None
    if B is None:
        mu, Q = numpy.linalg.eigh(GMs)
        keep = mu > s * numpy.finfo(float).eps * max(mu[-1], 0.0)
        keep &= mu > 0.0
        if not keep.any():
            raise ValueError('GM: numerically zero')
        B = Q[:, keep] / numpy.sqrt(mu[keep])
    H = B.T.dot(GAs).dot(B)
    theta, Z = numpy.linalg.eigh(0.5 * (H + H.T))
    C = scale[:, None] * B.dot(Z)
    return theta, C


def default_guard(k):
    return max(2, k // 4)


def check_block(k, guard, nfree):
    '''(k, guard, b) of a solve for k pairs on nfree free dofs.'''
    k = int(k)
    if k < 1:
        raise ValueError('k: at least one eigenpair')
    guard = default_guard(k) if guard is None else int(guard)
    if guard < 0:
        raise ValueError('guard: not negative')
    if k > nfree:
        raise ValueError('k = %d eigenpairs of a problem with %d free dofs'
                         % (k, nfree))
    if k + guard > MAX_BLOCK:
        raise ValueError('k + guard = %d columns; the block holds at most %d'
                         % (k + guard, MAX_BLOCK))
    # a block wider than the space is singular from the start
    b = min(k + guard, nfree)
    return k, b - k, b


def start_block(n, b, free, initial=None):
    '''The start block (n, b): fixed-seed normal numbers, the leading columns
    replaced by `initial` (arrays of n entries), zero off `free`.'''
    X = numpy.random.RandomState(SEED).standard_normal((n, b))
    for j, x in enumerate(initial or []):
        if j >= b:
            raise ValueError('initial: more than the %d columns of the block'
                             % b)
        X[:, j] = numpy.asarray(x, dtype=float).reshape(n)
    X[~free, :] = 0.0
    return X


class LoopResult(object):
    def __init__(self, values, residuals, converged, iterations):
        self.values, self.residuals = values, residuals
        self.converged, self.iterations = converged, iterations


def lobpcg(be, X0, k, rtol, maxit):
    '''LOBPCG on the backend `be` from the start block X0 (n, b); see the
    module's text.  Leaves the b Ritz vectors in the first b columns of the
    backend's current set (be.block()) and returns a LoopResult for all b
    columns (the caller keeps the first k).'''
    b = X0.shape[1]
    be.load(X0)
    be.apply(0, b)
    npc = nw = 0                   # columns of P and W in the current set
    theta = None
    res = numpy.full(b, numpy.inf)
    conv = numpy.zeros(b, dtype=bool)
    it = 0
    while True:
        s = b + npc + nw
        GA, GM, rr, mm = be.grams(s, theta is not None)
        if theta is not None:
            res = numpy.sqrt(numpy.maximum(rr, 0.0))
            ref = numpy.abs(theta[:k]).max()
            conv = res <= rtol * numpy.maximum(numpy.abs(theta), ref) \
                * numpy.sqrt(numpy.maximum(mm, 0.0))
            if conv[:k].all() or it >= maxit:
                break
        th, C = rayleigh_ritz(GA, GM)
        if len(th) < b:
            raise ValueError('the block lost rank: %d independent directions '
                             'for %d columns' % (len(th), b))
        theta = th[:b].copy()
        act = [j for j in range(b) if not conv[j]]
        rows = [C[:, :b].T]
        if s > b:
            # the part of the new iterate that came from P and W
            Cp = C[:, act].T.copy()
            Cp[:, :b] = 0.0
            rows.append(Cp)
            npc = len(act)
        else:
            npc = 0
        be.rotate(s, numpy.concatenate(rows, axis=0), theta)
        nw = len(act)
        be.expand(act, b + npc)
        be.apply(b + npc, nw)
        it += 1
    return LoopResult(theta, res, conv, it)


class HostBackend(object):
    '''The block operations of lobpcg in numpy / scipy: A, M scipy sparse
    (Dirichlet rows and columns already eliminated symmetrically), free: the
    boolean mask of the free dofs, precondition(R) -> W for a block.'''

    def __init__(self, A, M, free, b, precondition=None):
        self.A, self.M = A.tocsr(), M.tocsr()
        self.n = self.A.shape[0]
        self.free = numpy.asarray(free, dtype=bool)
        dinv = numpy.where(self.free, 1.0 / self.A.diagonal(), 0.0)
        self._T = precondition or (lambda R: dinv[:, None] * R)
        z = lambda: numpy.zeros((self.n, 3 * b))
        self.S, self.AS, self.MS = z(), z(), z()
        self.R = numpy.zeros((self.n, b))
        self.b = b

    def load(self, X0):
        self.S[:, :self.b] = X0

    def apply(self, j0, m):
        self.AS[:, j0:j0 + m] = self.A.dot(self.S[:, j0:j0 + m])
        self.MS[:, j0:j0 + m] = self.M.dot(self.S[:, j0:j0 + m])

    def grams(self, s, with_residuals):
        S, b = self.S[:, :s], self.b
        rr = mm = None
        if with_residuals:
            rr = (self.R * self.R).sum(axis=0)
            mm = (self.MS[:, :b] ** 2).sum(axis=0)
        return S.T.dot(self.AS[:, :s]), S.T.dot(self.MS[:, :s]), rr, mm

    def rotate(self, s, rows, theta):
        r, b = rows.shape[0], self.b
        new = []
        for T in (self.S, self.AS, self.MS):
            N = numpy.zeros_like(T)
            N[:, :r] = T[:, :s].dot(rows.T)
            new.append(N)
        self.S, self.AS, self.MS = new
        self.R = self.AS[:, :b] - self.MS[:, :b] * theta[None, :]

    def expand(self, act, j0):
        W = self._T(self.R[:, act])
        W[~self.free, :] = 0.0
        self.S[:, j0:j0 + len(act)] = W

    def block(self):
        return self.S[:, :self.b]


def host_eigensolve(A, M, free, k, rtol=1e-8, maxit=200, guard=None,
                    precondition=None):
    '''lobpcg with the HostBackend: (values (k,), X (n, k), LoopResult).'''
    free = numpy.asarray(free, dtype=bool)
    k, guard, b = check_block(k, guard, int(free.sum()))
    be = HostBackend(A, M, free, b, precondition)
    out = lobpcg(be, start_block(be.n, b, free), k, rtol, maxit)
    return out.values[:k], be.block()[:, :k].copy(), out


# -- the device backend ---------------------------------------------------------------
class DeviceBackend(object):
    '''The block operations of lobpcg on the device (see the module's text).
    A, M: Matrix objects of one kind (0, or 2 on a vector space) after the
    symmetric elimination; free: host boolean mask; precondition(r, z): one
    column, device tensors of A.size entries.'''

    # Matrix.apply_block against one flow_operator_apply per column: the
    # block product is used from this many columns on (measured: DESIGN.md);
    # BLOCK_FROM_2: the same for kind 2 (measured too: 0.95 at m = 1, 1.65 at
    # m = 2, tools/eigen_lab.py --vector)
    BLOCK_FROM = 2
    BLOCK_FROM_2 = 2

    def __init__(self, A, M, free, b, precondition):
        from .. import _hip, device
        self.A, self.M, self.b = A, M, b
        self.n = n = A.size
        self.ld = ld = n + (n & 1)
        self._T = precondition
        cols = 3 * b
        self.sets = [[device.zeros(cols * ld) for _ in range(3)]
                     for _ in range(2)]
        self.cur = 0
        self.R = device.zeros(b * ld)
        self._work = device.empty(cols * cols * _hip.MULTI_DOT_BLOCKS)
        self._out = device.zeros(2 * cols * cols + 2 * b * b)
        self.free = numpy.asarray(free, dtype=bool)

    def _col(self, T, j):
        return T[j * self.ld:j * self.ld + self.n]

    def load(self, X0):
        from .. import device
        n, b, ld = self.n, self.b, self.ld
        host = numpy.zeros((b, ld))
        host[:, :n] = X0.T
        S = self.sets[self.cur][0]
        S[:b * ld] = device.to_device(host.reshape(-1))

    def apply(self, j0, m):
        if m == 0:
            return
        S, AS, MS = self.sets[self.cur]
        ld, o = self.ld, j0 * self.ld
        for Mat, Y in ((self.A, AS), (self.M, MS)):
            if m >= (self.BLOCK_FROM_2 if Mat.kind == 2 else self.BLOCK_FROM):
                Mat.apply_block(S[o:], ld, m, Y[o:], ld)
            else:
                for j in range(j0, j0 + m):
                    Mat.apply(self._col(S, j), self._col(Y, j))

    def _gram(self, X, ma, Y, mb, out):
        from .. import _hip
        n, ld = self.n, self.ld
        _hip.check(_hip.lib().flow_block_gram(
            n, ma, _hip.f64(X, (ma - 1) * ld + n, 'X'), ld, mb,
            _hip.f64(Y, (mb - 1) * ld + n, 'Y'), ld,
            _hip.f64(self._work, ma * mb * _hip.MULTI_DOT_BLOCKS, 'work'),
            _hip.f64(out, ma * mb, 'out'), _hip.stream()))

    def grams(self, s, with_residuals):
        from .. import device
        S, AS, MS = self.sets[self.cur]
        b, out = self.b, self._out
        ss, bb = s * s, b * b
        self._gram(S, s, AS, s, out[:ss])
        self._gram(S, s, MS, s, out[ss:2 * ss])
        if with_residuals:
            self._gram(self.R, b, self.R, b, out[2 * ss:2 * ss + bb])
            self._gram(MS, b, MS, b, out[2 * ss + bb:2 * ss + 2 * bb])
        host = device.to_host(out[:2 * ss + 2 * bb]).numpy()
        GA = host[:ss].reshape(s, s).copy()
        GM = host[ss:2 * ss].reshape(s, s).copy()
        if not with_residuals:
            return GA, GM, None, None
        rr = numpy.diag(host[2 * ss:2 * ss + bb].reshape(b, b)).copy()
        mm = numpy.diag(host[2 * ss + bb:2 * ss + 2 * bb].reshape(b, b)).copy()
        return GA, GM, rr, mm

    def _combine(self, m, X, r, Cd, base, out):
        from .. import _hip
        n, ld = self.n, self.ld
        _hip.check(_hip.lib().flow_combine(
            n, m, _hip.f64(X, (m - 1) * ld + n, 'columns'), ld, r,
            _hip.f64(Cd, r * m, 'coefficients'),
            None if base is None else _hip.f64(base, n, 'base'),
            _hip.f64(out, (r - 1) * ld + n, 'out'), ld, _hip.stream()))

    def rotate(self, s, rows, theta):
        from .. import device
        r, b = rows.shape[0], self.b
        # one upload: the rotation and the -lambda_j of the residuals
        Cd = device.to_device(numpy.concatenate(
            [numpy.ascontiguousarray(rows, dtype=float).reshape(-1), -theta]))
        old, new = self.sets[self.cur], self.sets[1 - self.cur]
        for T, N in zip(old, new):
            self._combine(s, T, r, Cd[:r * s], None, N)
        self.cur = 1 - self.cur
        _, AS, MS = new
        for j in range(b):
            self._combine(1, self._col(MS, j), 1, Cd[r * s + j:r * s + j + 1],
                          self._col(AS, j), self._col(self.R, j))

    def expand(self, act, j0):
        S = self.sets[self.cur][0]
        for i, j in enumerate(act):
            self._T(self._col(self.R, j), self._col(S, j0 + i))

    def block(self):
        return self.sets[self.cur][0]


# -- the public interface ---------------------------------------------------------------
class vector_eigenmodes(_Switch):
    '''The switch of Eigenmodes on a P1 / P2 VectorFunctionSpace (2x2-block
    operators: vibration modes of an elastic body, the vector Laplacian).  Off
    by default: Eigenmodes of forms on a vector space stays the
    NotImplementedError it was.  `vector_eigenmodes(True)` switches it on at
    once, for the process; `.previous` is the setting it replaced, and as a
    context manager it restores that on exit.  `vector_eigenmodes.enabled` is
    the current setting.  The forms are written with test and trial functions
    on the vector space, so vector_arguments(True) is needed as well.'''
    enabled = False


def _no_strips():
    from .. import parallel
    if parallel.active():
        raise NotImplementedError(
            'Eigenmodes on strips is not implemented: a rank holds its own '
            'rows only')


def _check_forms(a, m, symmetric):
    '''The space of the rank-2 forms a and m (m may be None).'''
    from . import forms
    V = None
    for name, f in (('a', a), ('m', m)):
        if f is None:
            continue
        if not isinstance(f, forms.Form):
            raise TypeError('%s: a bilinear form (got %r)' % (name, type(f)))
        if f.rank != 2:
            raise ValueError('%s: a bilinear form (rank 2), not rank %d'
                             % (name, f.rank))
        W = f.arguments()[0]
        if forms.is_mixed_space(W):
            raise NotImplementedError(
                'Eigenmodes of forms on a mixed space is not implemented: '
                'LOBPCG takes positive definite problems on one scalar or '
                'vector space, a saddle-point operator is indefinite')
        if V is None:
            V = W
        elif not W.same_as(V):
            raise ValueError('a and m: forms on different spaces')
        for _, part in f.terms():
            if not symmetric and \
                    not forms.is_symmetric_table(part.argument_table()[1]):
                raise ValueError(
                    '%s: not symmetric in its test and trial functions as '
                    'written; LOBPCG takes symmetric problems only (pass '
                    'symmetric=True for a form that is symmetric all the '
                    'same)' % name)
    vector = getattr(V, 'component', None) is None and V.dim == 2
    if vector and not vector_eigenmodes.enabled:
        raise NotImplementedError(
            'Eigenmodes of forms on a vector space (2x2-block operators) is '
            'not implemented unless fem.vector_eigenmodes(True) switches it '
            'on: LOBPCG runs on scalar matrices only without it')
    if getattr(V, 'component', None) is not None \
            or (V.dim != 1 and not vector) or V.degree not in (1, 2):
        raise ValueError('a, m: forms on one scalar P1 or P2 space, or with '
                         'vector_eigenmodes(True) on one P1 or P2 vector space')
    return V


class EigenResult(object):
    '''values (k,) numpy ascending; modes: k Functions, M-orthonormal, the
    entry of largest magnitude positive; residuals (k,): |A x - lambda M x|_2;
    iterations; converged (k,) bool.'''

    def __init__(self, values, modes, residuals, iterations, converged):
        self.values, self.modes = values, modes
        self.residuals, self.iterations = residuals, iterations
        self.converged = converged


class Eigenmodes(object):
    '''The smallest eigenpairs of a == lambda m on one scalar P1 / P2 space,
    or with vector_eigenmodes(True) on one P1 / P2 VectorFunctionSpace (m
    None: dot(u, v)*dx; conditions on W and on W.sub(i)); see the module's
    text.'''

    def __init__(self, a, m=None, bcs=None, form_compiler_parameters=None,
                 symmetric=False):
        from . import forms, ops
        _no_strips()
        V = _check_forms(a, m, symmetric)
        if m is None and V.dim == 2:
            m = forms.dot(forms.TrialFunction(V), forms.TestFunction(V)) \
                * forms.dx
        elif m is None:
            m = forms.TrialFunction(V) * forms.TestFunction(V) * forms.dx
        _, _, mask = ops._scalar_bcs(bcs, V)
        A = ops.assemble(a, form_compiler_parameters)
        M = ops.assemble(m, form_compiler_parameters)
        self._setup(A, M, mask, V)

    @classmethod
    def from_matrices(cls, A, M, isbc=None):
        '''From assembled Matrix objects of one layout, both scalar (kind 0)
        or both 2x2-block (kind 2); isbc: the Dirichlet dofs as a boolean /
        0-1 array of A.size entries (N, or 2N in operator numbering; host or
        device), or None.'''
        from .. import device
        _no_strips()
        kinds = (getattr(A, 'kind', None), getattr(M, 'kind', None))
        if kinds not in ((0, 0), (2, 2)):
            raise ValueError('A, M: two scalar matrices (kind 0) or two '
                             '2x2-block matrices (kind 2)')
        if A.layout is not M.layout:
            raise ValueError('A, M: matrices of different layouts')
        mask = None
        if isbc is not None:
            host = isbc if isinstance(isbc, numpy.ndarray) or \
                isinstance(isbc, (list, tuple)) else \
                device.to_host(isbc).numpy()
            host = numpy.asarray(host).astype(bool)
            if host.shape != (A.size,):
                raise ValueError('isbc: one entry per dof')
            if host.any():
                mask = device.to_device(host.astype(numpy.uint8))
        self = cls.__new__(cls)
        self._setup(A, M, mask, None)
        return self

    def _setup(self, A, M, mask, V):
        from .. import device
        from . import ops
        self.V = V
        self.layout = A.layout
        n = A.size
        if mask is None:
            self.isbc = numpy.zeros(n, dtype=bool)
            self.A, self.M = A, M
        else:
            self.isbc = device.to_host(mask).numpy().astype(bool)
            eliminate = ops.symmetric_bc_blocks if A.kind == 2 else \
                ops.symmetric_bc_matrix
            self.A = eliminate(A, mask)
            self.M = eliminate(M, mask)
        self.free = ~self.isbc
        self._free_d = device.to_device(self.free.astype(numpy.float64))
        self._dinv = None
        self._coarse = None

    # -- preconditioners -------------------------------------------------------------
    def _jacobi(self):
        from . import ops
        if self._dinv is None:
            # zero on the Dirichlet dofs: W stays in the constrained subspace
            self._dinv = ops.vmul(self.A.diag_inv(), self._free_d)
        dinv = self._dinv
        return lambda r, z: ops.vmul(dinv, r, out=z)

    def _two_level(self):
        import ctypes
        from .. import _hip, device
        from . import ops
        self._jacobi()
        n = self.layout.N
        if self._coarse is None:
            # one scalar coarse space per component: on a vector space the
            # diagonal planes A_xx (0) and A_yy (3) of the eliminated matrix,
            # each with its half of the Dirichlet mask (the coupling planes
            # are ignored: z = [T_xx r_x ; T_yy r_y], block-diagonal and SPD)
            self._coarse = []
            for c, p in enumerate((0, 3) if self.A.kind == 2 else (0,)):
                Ac = self.A if self.A.kind == 0 else ops.Matrix(
                    self.layout, 0, self.A.vals[p * self.A.stride:
                                                (p + 1) * self.A.stride])
                isbc = self.isbc[c * n:(c + 1) * n]
                C = ops.CoarseSpace(Ac, isbc=isbc if isbc.any() else None,
                                    singular=not isbc.any())
                self._coarse.append((C, device.zeros(2 * C.struct.lda + 2)))
        coarse, dinv = self._coarse, self._dinv
        lib = _hip.lib()

        def apply(r, z):
            for c, (C, cwork) in enumerate(coarse):
                lo, hi = c * n, (c + 1) * n
                _hip.check(lib.flow_two_level_apply(
                    ctypes.byref(C.struct), _hip.f64(dinv[lo:hi], n),
                    _hip.f64(r[lo:hi], n), _hip.f64(z[lo:hi], n),
                    _hip.f64(cwork), _hip.stream()))
        return apply

    # -- the solve -------------------------------------------------------------------
    def solve(self, k, rtol=1e-8, maxit=200, guard=None,
              preconditioner='jacobi', initial=None,
              error_on_nonconvergence=True):
        '''The k smallest eigenpairs: an EigenResult.  _hip.NotConverged where
        fewer than k pairs meet rtol within maxit iterations, unless
        error_on_nonconvergence is False.'''
        from .. import _hip, device
        from .function import Function
        _no_strips()
        if preconditioner not in ('jacobi', 'two_level'):
            raise ValueError("preconditioner: 'jacobi' or 'two_level', not %r"
                             % (preconditioner,))
        n = self.A.size
        k, guard, b = check_block(k, guard, int(self.free.sum()))
        start = []
        for u in initial or []:
            if not isinstance(u, Function) or u.data.numel() != n:
                raise ValueError('initial: Functions of the space of the forms')
            start.append(device.to_host(u.data).numpy())
        T = self._jacobi() if preconditioner == 'jacobi' else self._two_level()
        be = DeviceBackend(self.A, self.M, self.free, b, T)
        out = lobpcg(be, start_block(n, b, self.free, start), k, float(rtol),
                     int(maxit))
        # the sign: the entry of largest magnitude (smallest index on ties)
        # positive -- the one read-back of the block
        ld = be.ld
        X = device.to_host(be.block()[:k * ld]).numpy().reshape(k, ld)[:, :n]
        sign = numpy.ones(k)
        for j in range(k):
            i = int(numpy.argmax(numpy.abs(X[j])))
            if X[j, i] < 0.0:
                sign[j] = -1.0
        buf = device.zeros(k * ld)
        be._combine(k, be.block(), k,
                    device.to_device(numpy.diag(sign).reshape(-1)), None, buf)
        V = self.V
        modes = [Function(V, buf[j * ld:j * ld + n]) if V is not None
                 else buf[j * ld:j * ld + n] for j in range(k)]
        res = EigenResult(out.values[:k].copy(), modes, out.residuals[:k].copy(),
                          out.iterations, out.converged[:k].copy())
        res._block = buf
        if error_on_nonconvergence and not res.converged.all():
            raise _hip.NotConverged(
                'Eigenmodes.solve: %d of %d pairs converged to rtol %g in %d '
                'iterations' % (int(res.converged.sum()), k, rtol,
                                out.iterations))
        return res

    def rayleigh(self, u):
        '''The Rayleigh quotient u^T A u / u^T M u of a Function (or a device
        tensor of N entries; 2N on a vector space) with the eliminated
        matrices.'''
        from .. import device
        from . import ops
        x = getattr(u, 'data', u)
        n = self.A.size
        y = device.empty(n)
        num = ops.dot(x, self.A.apply(x, y))
        den = ops.dot(x, self.M.apply(x, y))
        return num / den


def eigensolve(a, m=None, bcs=None, k=1, **kw):
    '''Eigenmodes(a, m, bcs).solve(k, ...) in one call; the keywords of the
    constructor (form_compiler_parameters, symmetric) and of solve().'''
    init = {key: kw.pop(key) for key in ('form_compiler_parameters', 'symmetric')
            if key in kw}
    return Eigenmodes(a, m, bcs, **init).solve(k, **kw)
