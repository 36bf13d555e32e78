# -*- coding: utf-8 -*-
'''
Nullspaces of singular problems: dolfin's VectorSpaceBasis, set_nullspace and
orthogonalize for solve(a == L, u, bcs, nullspace=ns) and solve(F == 0, w, bcs,
nullspace=ns).

    enclosed flow    velocity prescribed on the whole boundary: the pressure is
                     determined up to a constant -- constant_nullspace(WP);
    pure Neumann     Poisson without a Dirichlet condition: the constant --
                     constant_nullspace(V);
    a free body      elasticity under self-equilibrated tractions: the two
                     translations and the rotation -- rigid_body_modes(W).

A VectorSpaceBasis holds k <= 8 orthonormal columns in one column-major device
store with the layout flow_multi_dot takes (an even leading dimension, 16-byte
aligned columns) and, with `support`, the contiguous slice of the solution
vector they span: the pressure constant on a Taylor-Hood space has support
(2 Nv, Np), and the velocity part of a vector is then never streamed.

The projection x <- x - Z (Z^T x) is flow_deflate (csrc/nullspace_kernels.hip):
two launches, in place, no temporary and no host wait.  The solvers use it so:
the right-hand side and the start vector are projected once; the CG route of
scalar and vector spaces then runs the native CG untouched and projects the
result; the mixed loops (mixed.minres, mixed.fgmres, unchanged) get a
preconditioner wrapped by deflated_preconditioner, which projects every
preconditioned vector.  The left and the right nullspace must coincide (for
enclosed flow both are the pressure constant): one basis serves both, and that
is not checked.
'''
import numpy
import torch

from .function import Function, Vector
from .space import FunctionSpace, MixedFunctionSpace
from .. import _hip
from .. import device

MAX_DIM = 8
EPS = 2.0 ** -52


def _host_column(v):
    if isinstance(v, (Function, Vector)):
        v = v.data
    if isinstance(v, torch.Tensor):
        v = device.to_host(v).numpy()
    a = numpy.array(v, dtype=numpy.float64)
    if a.ndim != 1 or a.size == 0:
        raise ValueError('a basis vector is a non-empty one-dimensional array')
    return a


def _same_space(A, B):
    return type(A) is type(B) and A.same_as(B)


class VectorSpaceBasis(object):
    '''k <= 8 vectors (Functions, Vectors, device or host arrays of one
    length) that span a nullspace.  support = (offset, length): the vectors
    have `length` entries and stand for entries offset .. offset + length of
    the solution vector, zero elsewhere; default: the whole vector.  The space
    is taken from a Function among the vectors (or `space`); a basis without
    one is checked by its length alone.  The solvers take an orthonormal basis
    (orthonormalize()).'''

    def __init__(self, vectors, support=None, space=None):
        vectors = list(vectors)
        if not 1 <= len(vectors) <= MAX_DIM:
            raise ValueError('a basis holds 1 to %d vectors (got %d)'
                             % (MAX_DIM, len(vectors)))
        for v in vectors:
            if isinstance(v, Function):
                if space is not None and not _same_space(
                        space, v.function_space()):
                    raise ValueError('the basis vectors live on different '
                                     'spaces')
                space = v.function_space()
        cols = [_host_column(v) for v in vectors]
        n = cols[0].size
        if any(c.size != n for c in cols):
            raise ValueError('the basis vectors differ in length')
        if support is None:
            offset = 0
        else:
            offset, length = int(support[0]), int(support[1])
            if offset < 0 or length != n:
                raise ValueError('support (offset %d, length %d) does not fit '
                                 'vectors of %d entries' % (offset, length, n))
        if space is not None and offset + n > space.size():
            raise ValueError('the basis reaches past the %d entries of its '
                             'space' % space.size())
        if support is None and space is not None and n != space.size():
            raise ValueError('basis vectors of %d entries on a space of %d'
                             % (n, space.size()))
        self.space = space
        self.whole = support is None
        # the length of the solution vector, where the vectors say it
        self.length = n if self.whole else None
        Z = numpy.array(cols)
        if self.whole:
            # full-length vectors: the support is found -- the entries from
            # the first (rounded down to an even index: 16-byte alignment) to
            # the last one that is non-zero in some vector -- so that the same
            # basis gives the same bits however it was handed over
            nz = numpy.nonzero((Z != 0.0).any(axis=0))[0]
            if len(nz) == 0:
                raise ValueError('the basis vectors are all zero')
            offset = int(nz[0]) & ~1
            Z = numpy.ascontiguousarray(Z[:, offset:int(nz[-1]) + 1])
        self.offset, self.n = offset, Z.shape[1]
        self._Z = Z
        self._dev = None

    # -- host side ---------------------------------------------------------
    def dim(self):
        return self._Z.shape[0]

    @property
    def support(self):
        return (self.offset, self.n)

    def host(self):
        '''The columns as a (k, length) float64 host array (a copy).'''
        return self._Z.copy()

    def orthonormalize(self):
        '''Modified Gram-Schmidt on the host in float64 (two passes per
        vector), then one upload on first use.  A vector that depends on the
        ones before it is a ValueError.  Returns self.'''
        Z = self._Z.copy()
        for j in range(Z.shape[0]):
            scale = numpy.linalg.norm(Z[j])
            for _ in range(2):
                for i in range(j):
                    Z[j] -= Z[i].dot(Z[j]) * Z[i]
            nrm = numpy.linalg.norm(Z[j])
            if not nrm > 1.0e-10 * scale:
                raise ValueError('basis vector %d depends linearly on the '
                                 'ones before it' % j)
            Z[j] /= nrm
        self._Z = Z
        self._dev = None
        return self

    def gram_defect(self):
        '''max |Z^T Z - I| on the host.'''
        G = self._Z.dot(self._Z.T)
        return float(numpy.abs(G - numpy.eye(G.shape[0])).max())

    def is_orthonormal(self, tol=1.0e-12):
        return self.gram_defect() <= tol

    # -- device side -------------------------------------------------------
    def _store(self):
        if self._dev is None:
            k, n = self._Z.shape
            ld = n + (n & 1)
            host = numpy.zeros(k * ld)
            for j in range(k):
                host[j * ld:j * ld + n] = self._Z[j]
            store = device.to_device(host)
            assert store.data_ptr() % 16 == 0
            self._dev = (store, ld,
                         device.empty(k * _hip.MULTI_DOT_BLOCKS))
        return self._dev

    def _slice(self, x):
        data = x.data if isinstance(x, (Function, Vector)) else x
        if not isinstance(data, torch.Tensor):
            raise TypeError('a Vector, a Function or a device array')
        if isinstance(x, Function) and self.space is not None \
                and not _same_space(self.space, x.function_space()):
            raise ValueError('the basis lives on another space than the '
                             'Function')
        total = data.numel()
        want = self.space.size() if self.space is not None else self.length
        if (want is not None and total != want) \
                or total < self.offset + self.n:
            raise ValueError('a vector of %d entries against a basis on '
                             'entries %d .. %d%s'
                             % (total, self.offset, self.offset + self.n,
                                '' if want is None else ' of %d' % want))
        return data[self.offset:self.offset + self.n]

    def deflate(self, x, coef=None):
        '''x <- x - Z (Z^T x) on the support, in place (flow_deflate); coef:
        a device array that receives the k products Z^T x.  No host wait.'''
        xs = self._slice(x)
        store, ld, work = self._store()
        k, n = self._Z.shape
        _hip.check(_hip.lib().flow_deflate(
            n, k, _hip.f64(store, (k - 1) * ld + n, 'basis'), ld,
            _hip.f64(xs, n, 'x'), _hip.f64(work, k * _hip.MULTI_DOT_BLOCKS),
            None if coef is None else _hip.f64(coef, k, 'coef'),
            _hip.stream()))
        return x

    def orthogonalize(self, x):
        '''Remove the components of x along the basis, in place; x a Vector,
        a Function or a device array of the whole solution vector.'''
        self.deflate(x)
        return x

    def coefficients(self, x):
        '''Z^T x as a device array of k doubles (flow_multi_dot): no wait.'''
        xs = self._slice(x)
        store, ld, work = self._store()
        k, n = self._Z.shape
        out = device.empty(k)
        _hip.check(_hip.lib().flow_multi_dot(
            n, k, _hip.f64(store, (k - 1) * ld + n, 'basis'), ld,
            _hip.f64(xs, n, 'x'), _hip.f64(work, k * _hip.MULTI_DOT_BLOCKS),
            _hip.f64(out, k), _hip.stream()))
        return out

    def project_rhs(self, b):
        '''Project the right-hand side b (a device array) in place and leave
        what rhs_defect needs on the device: Z^T b and b . b from BEFORE the
        projection, k + 1 doubles.  No host wait; defect() reads them.'''
        k = self.dim()
        nb = b.numel()
        slots = device.empty(k + 1)
        _, _, work = self._store()
        self._slice(b)
        _hip.check(_hip.lib().flow_multi_dot(
            nb, 1, _hip.f64(b, nb, 'b'), nb + (nb & 1), _hip.f64(b, nb, 'b'),
            _hip.f64(work, _hip.MULTI_DOT_BLOCKS), _hip.f64(slots[k:], 1),
            _hip.stream()))
        self.deflate(b, slots)
        return slots

    @staticmethod
    def defect(slots):
        '''|Z^T b| / |b| of project_rhs's slots: the one read-back (after the
        solve, whose own last wait has drained the stream).  0 for b = 0.'''
        h = device.to_host(slots).numpy().astype(numpy.float64)
        bb = h[-1]
        return float(numpy.sqrt(h[:-1].dot(h[:-1]) / bb)) if bb > 0.0 else 0.0


def constant_nullspace(V):
    '''The normalised constant of a scalar P1 / P2 space, or, for a
    Taylor-Hood space WP, the normalised pressure constant with support
    (2 Nv, Np).'''
    if isinstance(V, MixedFunctionSpace):
        W, P = V.taylor_hood()
        z = numpy.full(P.N, 1.0 / numpy.sqrt(P.N))
        return VectorSpaceBasis([z], support=(W.size(), P.N), space=V)
    if not isinstance(V, FunctionSpace) or V.dim != 1 \
            or V.component is not None:
        raise ValueError('constant_nullspace takes a scalar space or a '
                         'Taylor-Hood space (rigid_body_modes is for vector '
                         'spaces)')
    return VectorSpaceBasis([numpy.full(V.N, 1.0 / numpy.sqrt(V.N))], space=V)


def rigid_body_modes(W):
    '''The two translations and the rotation (-y, x) of a P1 / P2 vector
    space at the dof coordinates, orthonormalised.  The rotation is a linear
    field: nodal interpolation is exact on both degrees.'''
    if not isinstance(W, FunctionSpace) or W.dim != 2:
        raise ValueError('rigid_body_modes takes a VectorFunctionSpace')
    c = W.layout.dof_coords
    N = W.N
    one, zero = numpy.ones(N), numpy.zeros(N)
    modes = [numpy.concatenate([one, zero]), numpy.concatenate([zero, one]),
             numpy.concatenate([-c[:, 1], c[:, 0]])]
    return VectorSpaceBasis(modes, space=W).orthonormalize()


# -- what the solvers call ---------------------------------------------------------
def validate(ns, V, bc_dofs):
    '''The checks of solve(..., nullspace=ns) that need no device; each a
    ValueError naming the cause.  V: the space of the unknown; bc_dofs: the
    Dirichlet dofs in the numbering of V (host array or None).'''
    if not isinstance(ns, VectorSpaceBasis):
        raise TypeError('nullspace= takes a fem.VectorSpaceBasis (got %r)'
                        % (type(ns),))
    defect = ns.gram_defect()
    if not defect <= 1.0e-12:
        raise ValueError('nullspace: the basis is not orthonormal (max |Z^T Z '
                         '- I| = %.3e): call orthonormalize()' % defect)
    if ns.space is not None and not _same_space(ns.space, V):
        raise ValueError('nullspace: the basis lives on another space than '
                         'the unknown')
    size = V.size()
    if ns.offset + ns.n > size or (ns.length is not None
                                   and ns.length != size):
        raise ValueError('nullspace: the basis has the wrong length (entries '
                         '%d .. %d against an unknown of %d entries)'
                         % (ns.offset, ns.offset + ns.n, size))
    if bc_dofs is not None and len(bc_dofs):
        d = numpy.asarray(bc_dofs, dtype=numpy.int64) - ns.offset
        d = d[(d >= 0) & (d < ns.n)]
        bad = d[(ns._Z[:, d] != 0.0).any(axis=0)]
        if len(bad):
            raise ValueError(
                'nullspace: a Dirichlet dof carries a non-zero entry of a '
                'basis vector (dof %d, %d in all): the constrained problem '
                'does not have this nullspace' % (bad[0] + ns.offset, len(bad)))


def _abs_copy(A):
    '''A matrix with the absolute values of A's entries (setup only).'''
    from . import mixed, ops
    if isinstance(A, mixed.MixedMatrix):
        rect = lambda B: None if B is None else mixed.RectMatrix(  # noqa: E731
            B.layout, torch.abs(B.vals))
        return mixed.MixedMatrix(
            A.space, None if A.uu is None else _abs_copy(A.uu),
            None if A.pp is None else _abs_copy(A.pp),
            [rect(B) for B in A.up], [rect(B) for B in A.pu])
    return ops.Matrix(A.layout, A.kind, torch.abs(A.vals))


def check_null(ns, A, threshold=None):
    '''|A z_j|_inf <= threshold |A|_inf |z_j|_inf for every basis vector
    (threshold None or True: sqrt(eps) -- a true null vector leaves rounding,
    a wrong one O(1); False: no check), a ValueError otherwise.  Setup: k + 1
    products and their norms are read back.'''
    from . import ops
    if threshold is False:
        return
    thr = numpy.sqrt(EPS) if threshold is None or threshold is True \
        else float(threshold)
    n = A.size
    one = device.zeros(n) + 1.0
    y = device.empty(n)
    anorm = ops.vector_norm(_abs_copy(A).apply(one, y), 'linf')
    Z = ns.host()
    for j in range(ns.dim()):
        full = numpy.zeros(n)
        full[ns.offset:ns.offset + ns.n] = Z[j]
        az = ops.vector_norm(A.apply(device.to_device(full), y), 'linf')
        bound = thr * anorm * numpy.abs(Z[j]).max()
        if not az <= bound:
            raise ValueError(
                'nullspace: basis vector %d is not in the nullspace of the '
                'assembled operator: |A z|_inf = %.3e > %.3e = %.3e |A|_inf '
                "|z|_inf (solver_parameters['nullspace_check'] overrides the "
                'threshold, False skips the check)' % (j, az, bound, thr))


def deflated_preconditioner(ns, precondition):
    '''precondition(v, z) followed by the projection of z.'''
    def apply(v, z):
        precondition(v, z)
        ns.deflate(z)
        return z
    return apply
