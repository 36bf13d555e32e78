# -*- coding: utf-8 -*-
'''
Reductions of a time series of fields that stays in HBM: the mean, the
energy-ranked structures (proper orthogonal decomposition, POD) and the
frequencies with their spatial modes (dynamic mode decomposition, DMD).

    S = Snapshots(V, capacity, inner='L2')   # V: scalar or 2-vector P1 / P2
    S.append(u, t=None)      # device copy + one Gram row; no synchronisation
    len(S); S.times; S.clear(); S.column(k, out=None); S.mean(out=None)
    S.gram()                 # (k, k) numpy, symmetric; synchronises
    pod = S.pod(r=None, rtol=1e-10, subtract_mean=True)
    dmd = S.dmd(r=None, rtol=1e-10, dt=None)

The store is one device tensor of capacity * ld doubles, column j at j * ld,
ld = V.dim * V.N rounded up to an even number (every column 16-byte aligned);
a column is a component-blocked dof vector, as Function.data is.

Everything follows from the columns, their Gram matrix G = X^T W X in the
chosen inner product, and linear combinations of the columns:

    inner     W                                          y of a Gram row
    'L2'      the consistent mass matrix of the scalar   y = M x
              layout (ops.assemble_mass), per component
    'lumped'  the vertex-rule mass (P1 only: on P2 its   y = w .* x
              edge rows vanish)
    'l2'      the identity                               y = x

append(u) for column k copies u, forms y_k and runs flow_multi_dot (csrc/
snapshot_kernels.hip) of the columns 0..k against y_k into row k of a device
capacity x capacity array; gram() reads the lower triangle back and mirrors
it, so G is exactly symmetric.  An entry depends on its two columns alone
(the kernel's summation order is fixed and does not involve the other
columns), so a row written at append time equals the same entries computed
later in a batch, bit for bit.

The small dense algebra is host numpy (pod_from_gram, dmd_from_gram: the
method of snapshots); modes, the mean and reconstructions are flow_combine
launches over the store.

Synchronisation.  append() never waits for the device.  gram() reads the Gram
array back.  mean(), pod(), dmd() and POD.reconstruct() upload their
coefficient matrix before the flow_combine launch, and an upload
synchronises (device.to_device); POD.project() reads its result back.

Limit.  The method of snapshots works on G, whose condition number is the
square of X's: structures below about 1e-8 sigma_1 (lambda below 1e-16
lambda_1) are rounding in G and cannot be recovered.  That is why `rtol` acts
on the eigenvalues lambda = sigma^2, and why its default is 1e-10.

Not on strips.
'''
import math

import numpy

INNER = ('L2', 'lumped', 'l2')


# -- host algebra (numpy only) ------------------------------------------------------
def _rank(lam, r, rtol):
    '''How many of the descending eigenvalues lam to keep: those above rtol *
    lam[0] (and above zero), at most r.'''
    if len(lam) == 0 or not lam[0] > 0.0:
        return 0
    keep = int(numpy.count_nonzero(lam > rtol * lam[0]))
    return keep if r is None else min(keep, int(r))


def _sym_eig(G):
    '''Eigenpairs of the symmetric G, eigenvalues descending.'''
    lam, V = numpy.linalg.eigh(0.5 * (G + G.T))
    return lam[::-1].copy(), V[:, ::-1].copy()


def pod_from_gram(G, r=None, rtol=1e-10, subtract_mean=True):
    '''POD by the method of snapshots from the Gram matrix G = X^T W X (k, k).

    Returns (energies, C, a): all eigenvalues of the (centred) Gram matrix,
    descending; the coefficient matrix C (k, r) = H V Lambda^-1/2 whose
    columns combine the snapshots into the modes X C, orthonormal in W; the
    temporal coefficients a (r, k) = Lambda^1/2 V^T, so that X H = (X C) a.
    H = I - 1 1^T / k where subtract_mean, else I.  Kept: lambda_i > rtol *
    lambda_1, at most r.'''
    G = numpy.asarray(G, dtype=float)
    k = G.shape[0]
    if G.shape != (k, k) or k < 1:
        raise ValueError('G: a square matrix of at least one snapshot')
    if r is not None and int(r) < 1:
        raise ValueError('r: at least one mode')
    H = numpy.eye(k)
    if subtract_mean:
        H -= 1.0 / k
    lam, V = _sym_eig(H.dot(G).dot(H))
    nr = _rank(lam, r, rtol)
    root = numpy.sqrt(lam[:nr])
    C = H.dot(V[:, :nr]) / root
    a = root[:, None] * V[:, :nr].T
    return lam, C, a


def dmd_from_gram(G, r=None, rtol=1e-10):
    '''Exact DMD by the method of snapshots from the Gram matrix G (k, k) of
    k >= 2 snapshots: with X0 = X[:, :-1], X1 = X[:, 1:], G11 = G[:-1, :-1] =
    V Sigma^2 V^T and G12 = G[:-1, 1:],

        Atilde = Sigma^-1 V^T G12 V Sigma^-1,   eig(Atilde) = (Lambda, W).

    Returns (eigenvalues Lambda (r,) complex, T (k-1, r) complex, amplitudes
    b (r,) complex, sigma2): the exact modes are X1 T with T = V Sigma^-1 W
    Lambda^-1, b = W^-1 Sigma V^T e_0 expands the first snapshot in the
    projected modes, sigma2 are all eigenvalues of G11 (descending).  Kept:
    sigma2_i > rtol * sigma2_1, at most r.'''
    G = numpy.asarray(G, dtype=float)
    k = G.shape[0]
    if G.shape != (k, k) or k < 2:
        raise ValueError('G: a square matrix of at least two snapshots')
    if r is not None and int(r) < 1:
        raise ValueError('r: at least one mode')
    s2, V = _sym_eig(G[:-1, :-1])
    nr = _rank(s2, r, rtol)
    if nr == 0:
        raise ValueError('the snapshots vanish: no mode to keep')
    V = V[:, :nr]
    sig = numpy.sqrt(s2[:nr])
    At = (V.T.dot(G[:-1, 1:]).dot(V)) / sig[:, None] / sig[None, :]
    lam, W = numpy.linalg.eig(At)
    T = (V / sig).dot(W) / lam
    b = numpy.linalg.solve(W, (sig * V[0, :]).astype(complex))
    return lam, T, b, s2


def resolve_dt(dt, times):
    '''The time step of a DMD: `dt` where given, else the spacing of `times`
    (one per snapshot, none of them None) where that is uniform (ValueError
    where it is not), else None.'''
    if dt is not None:
        dt = float(dt)
        if not dt > 0.0:
            raise ValueError('dt: a positive time step')
        return dt
    if not times or any(t is None for t in times) or len(times) < 2:
        return None
    d = numpy.diff(numpy.asarray(times, dtype=float))
    if not (d > 0.0).all() or \
            numpy.abs(d - d[0]).max() > 1e-9 * numpy.abs(d).max():
        raise ValueError('times: not uniformly spaced; pass dt for the step '
                         'the snapshots are meant to be apart')
    return float((times[-1] - times[0]) / (len(times) - 1))


# -- the space ----------------------------------------------------------------------
def _no_strips():
    from .. import parallel
    if parallel.active():
        raise NotImplementedError(
            'Snapshots on strips is not implemented: a rank holds its own '
            'rows only')


def _check_space(V, inner):
    if not hasattr(V, 'layout'):
        raise NotImplementedError(
            'V: a mixed space; store the fields of its sub-spaces one by one')
    if getattr(V, 'component', None) is not None:
        raise NotImplementedError(
            'V: a component view (W.sub(i)); store the vector field, or '
            'Functions on W.sub(i).collapse()')
    if V.degree not in (1, 2):
        raise ValueError('V: P%r; snapshots take P1 or P2' % (V.degree,))
    if V.dim not in (1, 2):
        raise ValueError('V: %r components; scalar or 2-vector' % (V.dim,))
    if inner not in INNER:
        raise ValueError('inner: %r; one of %r' % (inner, INNER))
    if inner == 'lumped' and V.degree != 1:
        raise ValueError("inner: 'lumped' is the vertex-rule mass, whose P2 "
                         "edge rows vanish; P1 only (use 'L2')")
    _no_strips()


class _Weight(object):
    '''y = W x for dof vectors of V, W by `inner` (see the module's text).'''

    def __init__(self, V, inner):
        self.V, self.inner = V, inner
        self._M = self._w = self._stage = None

    def apply(self, x, y):
        '''W x into y (device tensors of dim * N doubles, x != y); returns
        the tensor that holds W x: y, or x itself for 'l2'.'''
        from .. import _hip, device
        from . import ops
        V, N = self.V, self.V.N
        if self.inner == 'l2':
            return x
        if self.inner == 'lumped':
            if self._w is None:
                # the diagonal of the vertex-rule mass: its product with ones
                D = ops.assemble_scalar_matrix(V.layout, ops.LUMPED_MASS)
                one = _hip.fill(device.empty(N), 1.0)
                d = D.apply(one, device.empty(N))
                w = device.empty(V.dim * N)
                for c in range(V.dim):
                    _hip.copy(w[c * N:(c + 1) * N], d)
                self._w = w
            return ops.vmul(self._w, x, out=y)
        if self._M is None:
            self._M = ops.assemble_mass(V)
        for c in range(V.dim):
            xc, yc = x[c * N:(c + 1) * N], y[c * N:(c + 1) * N]
            if xc.data_ptr() % 16 == 0 and yc.data_ptr() % 16 == 0:
                self._M.apply(xc, yc)
                continue
            # an odd N puts the second component 8 bytes off: through
            # aligned buffers
            if self._stage is None:
                self._stage = (device.empty(N), device.empty(N))
            sx, sy = self._stage
            self._M.apply(_hip.copy(sx, xc), sy)
            _hip.copy(yc, sy)
        return y


def _multi_dot(n, m, X, ld, y, work, out):
    '''flow_multi_dot of the first m columns of the store X (tensor, column
    stride ld) against y into the device tensor out (>= m doubles); work: m *
    MULTI_DOT_BLOCKS doubles.'''
    from .. import _hip
    lib = _hip.lib()
    _hip.check(lib.flow_multi_dot(
        n, m, _hip.f64(X, (m - 1) * ld + n, 'columns'), ld,
        _hip.f64(y, n, 'y'),
        _hip.f64(work, m * _hip.MULTI_DOT_BLOCKS, 'work'),
        _hip.f64(out, m, 'out'), _hip.stream()))
    return out


def _combine(n, m, X, ld, C, base, out, ldo):
    '''flow_combine: the rows of the host matrix C (r, m) combine the first m
    columns of X into the r columns of out (tensor, column stride ldo).  The
    upload of C synchronises.'''
    from .. import _hip, device
    lib = _hip.lib()
    C = numpy.ascontiguousarray(C, dtype=numpy.float64)
    r = C.shape[0]
    assert C.shape == (r, m)
    Cd = device.to_device(C.reshape(-1))
    _hip.check(lib.flow_combine(
        n, m, _hip.f64(X, (m - 1) * ld + n, 'columns'), ld, r,
        _hip.f64(Cd, r * m, 'coefficients'),
        None if base is None else _hip.f64(base, n, 'base'),
        _hip.f64(out, (r - 1) * ldo + n, 'out'), ldo, _hip.stream()))
    return out


class Snapshots(object):
    '''Up to `capacity` Functions of V (scalar or 2-vector P1 / P2) kept in
    HBM with their Gram matrix in the inner product `inner`; see the module's
    text.'''

    def __init__(self, V, capacity, inner='L2'):
        from .. import _hip, device
        _check_space(V, inner)
        capacity = int(capacity)
        if capacity < 1:
            raise ValueError('capacity: at least one snapshot')
        self.V, self.capacity, self.inner = V, capacity, inner
        self.n = V.dim * V.N
        self.ld = self.n + (self.n & 1)
        self._X = device.empty(capacity * self.ld)
        self._G = device.zeros(capacity * capacity)
        self._y = device.empty(self.ld)
        # the block partials of a Gram row: the store's own, of fixed size
        # and address, so that append() allocates nothing
        self._work = device.empty(capacity * _hip.MULTI_DOT_BLOCKS)
        self._weight = _Weight(V, inner)
        self._times = []

    # -- the store ----------------------------------------------------------------
    def __len__(self):
        return len(self._times)

    @property
    def times(self):
        '''The `t` of every append (None where none was given), in order.'''
        return list(self._times)

    def clear(self):
        '''Forget the snapshots (the store and its capacity stay).'''
        self._times = []

    def _check_u(self, u, what='u'):
        from .function import Function
        if not isinstance(u, Function) \
                or not u.function_space().same_as(self.V):
            raise ValueError('%s: not a Function of the space these '
                             'snapshots were built for' % what)

    def _col(self, k):
        return self._X[k * self.ld:k * self.ld + self.n]

    def _gram_row(self, k):
        '''Row k of the device Gram array: columns 0..k against W x_k.'''
        y = self._weight.apply(self._col(k), self._y[:self.n])
        _multi_dot(self.n, k + 1, self._X, self.ld, y, self._work,
                   self._G[k * self.capacity:(k + 1) * self.capacity])

    def append(self, u, t=None):
        '''Store the Function u as the next column (time t, optional) and
        fill its row of the Gram array: a device copy, the weighting and one
        flow_multi_dot on the package's stream, no host synchronisation.'''
        from .. import _hip
        _no_strips()
        self._check_u(u)
        k = len(self._times)
        if k >= self.capacity:
            raise ValueError('the store is full (capacity %d); clear() it or '
                             'build a larger one' % self.capacity)
        _hip.copy(self._col(k), u.data)
        self._gram_row(k)
        self._times.append(None if t is None else float(t))

    def _out(self, out):
        from .function import Function
        if out is None:
            return Function(self.V)
        self._check_u(out, 'out')
        return out

    def column(self, k, out=None):
        '''Snapshot k as a Function of V (a copy; into `out` where given).'''
        from .. import _hip
        if not 0 <= k < len(self):
            raise IndexError('snapshot %r of %d' % (k, len(self)))
        out = self._out(out)
        _hip.copy(out.data, self._col(k))
        return out

    def mean(self, out=None):
        '''The mean of the snapshots as a Function of V: one flow_combine.'''
        k = len(self)
        if k == 0:
            raise ValueError('no snapshots')
        out = self._out(out)
        _combine(self.n, k, self._X, self.ld, numpy.full((1, k), 1.0 / k),
                 None, out.data, self.ld)
        return out

    def gram(self):
        '''G[i, j] = <x_i, x_j> in the inner product, (k, k) numpy and exactly
        symmetric: the lower triangle the appends wrote, mirrored.  One
        read-back (synchronises).'''
        from .. import device
        k, cap = len(self), self.capacity
        full = device.to_host(self._G).numpy().reshape(cap, cap)[:k, :k]
        low = numpy.tril(full)
        return low + numpy.tril(full, -1).T

    # -- the decompositions ----------------------------------------------------------
    def _block(self, C, m, first=0):
        '''The columns first..first+m of the store combined by the rows of C
        (r, m): a tensor of r * ld doubles and the r Functions that view it.'''
        from .. import device
        from .function import Function
        r = C.shape[0]
        buf = device.empty(r * self.ld)
        _combine(self.n, m, self._X[first * self.ld:], self.ld, C, None, buf,
                 self.ld)
        return buf, [Function(self.V, buf[i * self.ld:i * self.ld + self.n])
                     for i in range(r)]

    def pod(self, r=None, rtol=1e-10, subtract_mean=True):
        '''The POD of the stored snapshots (about their mean where
        subtract_mean): a POD object.  Modes with lambda_i > rtol * lambda_1,
        at most r.'''
        k = len(self)
        if k == 0:
            raise ValueError('no snapshots')
        lam, C, a = pod_from_gram(self.gram(), r, rtol, subtract_mean)
        if C.shape[1] == 0:
            raise ValueError('the (centred) snapshots vanish: no mode to keep')
        buf, modes = self._block(C.T, k)
        return POD(self, lam, a, buf, modes,
                   self.mean() if subtract_mean else None)

    def dmd(self, r=None, rtol=1e-10, dt=None):
        '''The exact DMD of the stored snapshots, taken as one sequence a
        fixed step apart: a DMD object.  dt: that step, for frequencies and
        growth rates; without it the spacing of `times` where every append
        gave one (ValueError where they are not uniform).'''
        k = len(self)
        if k < 2:
            raise ValueError('a DMD needs at least two snapshots')
        step = resolve_dt(dt, self._times)
        lam, T, b, _ = dmd_from_gram(self.gram(), r, rtol)
        nr = len(lam)
        C = numpy.concatenate([T.real.T, T.imag.T], axis=0)       # (2 r, k - 1)
        _, fs = self._block(C, k - 1, first=1)
        return DMD(lam, b, [(fs[i], fs[nr + i]) for i in range(nr)], step)


class POD(object):
    '''energies: all eigenvalues of the (centred) Gram matrix, descending;
    r: modes kept; modes: r Functions of V, orthonormal in the inner product
    (views of one block); coefficients (r, k): snapshot j is mean + sum_i
    coefficients[i, j] * modes[i] (to the truncation); mean: a Function, or
    None where the mean was not subtracted.'''

    def __init__(self, store, energies, coefficients, block, modes, mean):
        self._store, self._block = store, block
        self.energies = energies
        self.coefficients = coefficients
        self.modes = modes
        self.r = len(modes)
        self.mean = mean

    def project(self, u):
        '''The r coefficients <modes[i], u - mean> (numpy): the weighting of
        u - mean and one flow_multi_dot over the mode block.'''
        from .. import _hip, device
        from . import ops
        S = self._store
        S._check_u(u)
        d = _hip.clone(u.data)
        if self.mean is not None:
            ops.axpby(-1.0, self.mean.data, 1.0, d)
        y = S._weight.apply(d, S._y[:S.n])
        out = _multi_dot(S.n, self.r, self._block, S.ld, y, S._work,
                         device.empty(self.r))
        return device.to_host(out).numpy().copy()

    def reconstruct(self, a, out=None):
        '''mean + sum_i a[i] * modes[i] as a Function of V (into `out` where
        given): one flow_combine.'''
        S = self._store
        a = numpy.asarray(a, dtype=float).reshape(-1)
        if a.shape != (self.r,):
            raise ValueError('a: %d coefficients, one per mode' % self.r)
        out = S._out(out)
        _combine(S.n, self.r, self._block, S.ld, a[None, :],
                 None if self.mean is None else self.mean.data, out.data, S.ld)
        return out


class DMD(object):
    '''eigenvalues (r,) complex: the factors per step; modes: r pairs (re,
    im) of Functions of V; amplitudes (r,) complex: the first snapshot in the
    modes; dt: the step, or None.'''

    def __init__(self, eigenvalues, amplitudes, modes, dt):
        self.eigenvalues = numpy.asarray(eigenvalues, dtype=complex)
        self.amplitudes = numpy.asarray(amplitudes, dtype=complex)
        self.modes = modes
        self.r = len(self.eigenvalues)
        self.dt = dt

    def _step(self):
        if self.dt is None:
            raise ValueError(
                'no time step: pass dt to dmd(), or a time to every append()')
        return self.dt

    @property
    def frequencies(self):
        '''Im log(lambda) / (2 pi dt): cycles per unit time, signed.'''
        return numpy.log(self.eigenvalues).imag / (2.0 * math.pi * self._step())

    @property
    def growth_rates(self):
        '''Re log(lambda) / dt.'''
        return numpy.log(self.eigenvalues).real / self._step()
