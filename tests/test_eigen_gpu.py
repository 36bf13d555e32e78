# -*- coding: utf-8 -*-
'''
fem.Eigenmodes on the device: the two block kernels against the kernels whose
bits they promise, and the eigensolver against eigen_reference (scipy's direct
solvers on the matrices read back from the device).

Bounds (every test prints its measured error next to its bound, pytest -s):

apply_block      every column bit-equal to flow_operator_apply on that column
                 (torch.equal), the padding of Y untouched.
flow_block_gram  every entry bit-equal to flow_multi_dot of the same columns;
                 two calls bit-equal.
eigenvalues      a returned lambda_j lies within |r_j|_2 / (sqrt(lambda_min(
                 M_free)) |x_j|_M) of an eigenvalue (Krylov-Weinstein), r_j
                 recomputed on the host from the matrices read back; on top,
                 the reference's own error: 1e3 eps lambda_k for the direct
                 solvers (eigh; eigsh at tol 1e-13).  The k reference values
                 are each matched once.
X^T M X - I      (n + 32) eps | |X|^T |M| |X| |, the Gram bound of
                 test_snapshots_gpu.py.
residuals        reported against recomputed: the rounding of the recomputed
                 one, (nnz per row + 2) eps (|A| |x| + |lambda| |M| |x|) per
                 entry, in the 2-norm, times 2 for the device's own.
'''
import ctypes
import functools

import numpy
import pytest
import torch

from flow_amd import _hip, device, fem
from flow_amd.fem import ops

import eigen_reference as eref

pytestmark = pytest.mark.gpu

EPS = numpy.finfo(float).eps
KRED = 1024
MC = 2                       # kBlockMC of csrc/eigen_kernels.hip


def _report(what, err, bound):
    print('%s: error %.2e  bound %.2e' % (what, err, bound))
    assert numpy.isfinite(err) and err <= bound


# -- 1. apply_block ----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _matrix(which):
    if which == 'p1-tiny':
        V = fem.FunctionSpace(fem.UnitSquareMesh(1, 1), 'P', 1)
    elif which == 'p1':
        V = fem.FunctionSpace(fem.UnitSquareMesh(20, 20), 'P', 1)
    elif which == 'p2':
        V = fem.FunctionSpace(fem.UnitSquareMesh(20, 20), 'P', 2)
    else:
        V = fem.FunctionSpace(fem.karman_channel_graded(lcar=1.0e-2), 'P', 2)
    return V, ops.assemble_stiffness(V)


@pytest.mark.parametrize('chunk', [0, 2, 4, 8])
@pytest.mark.parametrize('which', ['p1-tiny', 'p1', 'p2', 'graded'])
def test_apply_block_bits(hip, which, chunk):
    V, A = _matrix(which)
    n = V.N
    if which == 'p1-tiny':
        assert n == 4
    if which == 'p2':
        assert n == 1681 and A.operator().nblocks > 1
    mmax = 2 * 8 + 1
    ldx, ldy = (n + 3) & ~1, (n + 5) & ~1
    rng = numpy.random.RandomState(n % 997)
    X = numpy.full((mmax, ldx), numpy.nan)
    X[:, :n] = rng.uniform(-1.0, 1.0, size=(mmax, n))
    Xd = device.to_device(X.reshape(-1))
    mc = chunk or MC
    for m in sorted(set([1, 3, mc, mc + 1, 2 * mc + 1])):
        Yd = device.empty(mmax * ldy)
        Yd.fill_(-7.0)
        A.apply_block(Xd, ldx, m, Yd, ldy, chunk=chunk)
        Y = Yd.reshape(mmax, ldy)
        for j in range(m):
            want = A.apply(Xd[j * ldx:j * ldx + n].clone(), device.empty(n))
            assert torch.equal(Y[j, :n], want), (which, m, j)
        assert bool((Y[:m, n:] == -7.0).all()) and bool((Y[m:] == -7.0).all())
        assert bool(torch.isfinite(Y[:m, :n]).all())
    print('%s (n %d, %d row blocks) chunk %d: all columns bit-equal'
          % (which, n, A.operator().nblocks, mc))


def test_apply_block_refusals(hip):
    V, A = _matrix('p1')
    n = V.N
    ld = n + (n & 1)
    X = device.zeros(4 * ld + 2)
    Y = device.zeros(4 * ld + 2)
    M2 = ops.Matrix(V.layout, 1)         # (its zero fill is a launch)
    before = _hip.launch_count()
    op = ctypes.byref(A.operator())
    st = _hip.stream()

    def call(m, x, ldx, y, ldy, mc=0):
        return hip.flow_operator_apply_block_chunk(
            op, m, _hip.f64(x), ldx, _hip.f64(y), ldy, mc, st)
    assert call(2, X, ld - 2, Y, ld) == 2           # ldx < n
    assert call(2, X, ld + 1, Y, ld + 2) == 2       # odd ldx
    assert call(2, X[1:], ld, Y, ld) == 2           # misaligned X
    assert call(2, X, ld, Y[1:], ld) == 2           # misaligned Y
    assert call(2, X, ld, X[ld:], ld) == 2          # Y overlaps X
    assert call(2, X, ld, Y, ld, 3) == 2            # chunk
    with pytest.raises(ValueError):
        M2.apply_block(X, ld, 1, Y, ld)
    assert hip.flow_operator_apply_block(
        ctypes.byref(M2.operator()), 1, _hip.f64(X), ld, _hip.f64(Y), ld,
        st) == 2
    assert call(0, X, ld, Y, ld) == 0               # nothing to do
    assert _hip.launch_count() == before


# -- 2. flow_block_gram ------------------------------------------------------------------
GRAM_N = [1, 255, 257, 4099, KRED * 256 + 1]
MMAX = 17


@functools.lru_cache(maxsize=2)
def _blocks(n):
    rng = numpy.random.RandomState(n % 1000 + 3)
    ldx, ldy = (n + 3) & ~1, (n + 7) & ~1
    X = numpy.full((MMAX, ldx), numpy.nan)
    Y = numpy.full((MMAX, ldy), numpy.nan)
    X[:, :n] = rng.uniform(-1.0, 1.0, size=(MMAX, n))
    Y[:, :n] = rng.uniform(-1.0, 1.0, size=(MMAX, n))
    return (X, Y, device.to_device(X.reshape(-1)), ldx,
            device.to_device(Y.reshape(-1)), ldy)


def _gram(lib, n, ma, Xd, ldx, mb, Yd, ldy):
    out = device.empty(ma * mb)
    out.fill_(float('nan'))
    work = device.empty(ma * mb * KRED)
    _hip.check(lib.flow_block_gram(
        n, ma, _hip.f64(Xd, (ma - 1) * ldx + n), ldx, mb,
        _hip.f64(Yd, (mb - 1) * ldy + n), ldy, _hip.f64(work),
        _hip.f64(out, ma * mb), _hip.stream()))
    return device.to_host(out).numpy().reshape(ma, mb)


@pytest.mark.parametrize('n', GRAM_N)
def test_block_gram_bits(hip, n):
    X, Y, Xd, ldx, Yd, ldy = _blocks(n)
    for ma, mb in [(1, 1), (3, 5), (9, 8), (17, 17)]:
        got = _gram(hip, n, ma, Xd, ldx, mb, Yd, ldy)
        again = _gram(hip, n, ma, Xd, ldx, mb, Yd, ldy)
        assert numpy.array_equal(got.view(numpy.int64), again.view(numpy.int64))
        want = numpy.empty((ma, mb))
        work = device.empty(ma * KRED)
        for j in range(mb):
            out = device.empty(ma)
            _hip.check(hip.flow_multi_dot(
                n, ma, _hip.f64(Xd, (ma - 1) * ldx + n), ldx,
                _hip.f64(Yd[j * ldy:], n), _hip.f64(work), _hip.f64(out, ma),
                _hip.stream()))
            want[:, j] = device.to_host(out).numpy()
        assert numpy.array_equal(got.view(numpy.int64), want.view(numpy.int64))
        exact = X[:ma, :n].dot(Y[:mb, :n].T)
        bound = n * EPS * numpy.abs(X[:ma, :n]).dot(numpy.abs(Y[:mb, :n]).T)
        _report('n %d (%d, %d): bit-equal to flow_multi_dot; error / bound '
                'against numpy' % (n, ma, mb),
                (numpy.abs(got - exact) / bound).max(), 1.0)


def test_block_gram_refusals(hip):
    n = 100
    X = device.zeros(4 * n + 2)
    Y = device.zeros(4 * n + 2)
    work = device.zeros(16 * KRED)
    out = device.zeros(16)
    st = _hip.stream()
    before = _hip.launch_count()

    def call(x, ldx, y, ldy, w=work, o=out, ma=2, mb=2):
        return hip.flow_block_gram(n, ma, _hip.f64(x), ldx, mb, _hip.f64(y),
                                   ldy, _hip.f64(w), _hip.f64(o), st)
    assert call(X, n - 2, Y, n) == 2
    assert call(X, n + 1, Y, n) == 2
    assert call(X, n, Y, n + 1) == 2
    assert call(X[1:], n, Y, n) == 2
    assert call(X, n, Y[1:], n) == 2
    assert call(X, n, Y, n, o=X[n:]) == 2           # out inside X
    assert call(X, n, Y, n, w=Y) == 2               # work over Y
    assert call(X, n, Y, n, o=work[2:]) == 2        # out inside work
    assert call(X, n, Y, n, ma=0) == 0
    assert _hip.launch_count() == before
    assert call(X, n, X, n) == 0                    # X against itself is fine


# -- 3. the eigensolver ------------------------------------------------------------------
def _problem(which):
    '''(a, m, bcs, V) of the named problem.'''
    if which in ('dirichlet-p1', 'dirichlet-p2', 'neumann'):
        V = fem.FunctionSpace(fem.UnitSquareMesh(16, 16), 'P',
                              2 if which == 'dirichlet-p2' else 1)
        u, v = fem.TrialFunction(V), fem.TestFunction(V)
        a = fem.inner(fem.grad(u), fem.grad(v)) * fem.dx
        bcs = None if which == 'neumann' else \
            [fem.DirichletBC(V, 0.0, 'on_boundary')]
        return a, None, bcs, V
    mesh = fem.rectangle_with_hole(0.0, 2.0, 0.0, 1.0, (0.7, 0.5), 0.2, 24, 12)
    V = fem.FunctionSpace(mesh, 'P', 1)
    u, v = fem.TrialFunction(V), fem.TestFunction(V)
    x = fem.SpatialCoordinate(mesh)
    c = 1.0 + 20.0 * x[0] * x[0] + fem.sin(3.0 * x[1])
    a = fem.inner(fem.grad(u), fem.grad(v)) * fem.dx + c * u * v * fem.dx
    bcs = [fem.DirichletBC(V, 0.0, lambda p, on: on and p[0] < 1e-10)]
    return a, u * v * fem.dx, bcs, V


@functools.lru_cache(maxsize=None)
def _reference(which, k):
    '''The unconstrained host matrices as the device assembled them, the
    Dirichlet mask, lambda_min(M_free) and the reference eigenpairs.'''
    a, m, bcs, V = _problem(which)
    if m is None:
        m = fem.TrialFunction(V) * fem.TestFunction(V) * fem.dx
    A = fem.assemble(a).to_scipy()
    M = fem.assemble(m).to_scipy()
    isbc = numpy.zeros(V.N, dtype=bool)
    _, _, mask = ops._scalar_bcs(bcs, V)
    if mask is not None:
        isbc = device.to_host(mask).numpy().astype(bool)
    want, Xr = eref.smallest(A, M, isbc, k + 2)
    return A, M, isbc, eref.mass_lambda_min(M, isbc), want, Xr


CASES = [('dirichlet-p1', 6), ('dirichlet-p2', 6), ('neumann', 4),
         ('coefficient', 5)]


@pytest.mark.parametrize('preconditioner', ['jacobi', 'two_level'])
@pytest.mark.parametrize('which,k', CASES)
def test_eigenmodes_against_reference(hip, which, k, preconditioner):
    a, m, bcs, V = _problem(which)
    A, M, isbc, lmin, want, _ = _reference(which, k)
    E = fem.Eigenmodes(a, m, bcs)
    r = E.solve(k, rtol=1e-9, maxit=400, preconditioner=preconditioner)
    print('%s %s: %d iterations, values %s' % (which, preconditioner,
                                                r.iterations, r.values))
    assert r.converged.all() and len(r.modes) == k
    assert (numpy.diff(r.values) >= 0.0).all()
    X = numpy.stack([device.to_host(u.data).numpy() for u in r.modes], axis=1)
    n = V.N
    # the modes vanish exactly on the Dirichlet dofs; the sign convention
    assert (X[isbc, :] == 0.0).all()
    for j in range(k):
        i = int(numpy.argmax(numpy.abs(X[:, j])))
        assert X[i, j] > 0.0
    # on vectors that vanish there, the unconstrained matrices act as the
    # eliminated ones on the free rows
    f = (~isbc).astype(float)[:, None]
    AX, MX = f * A.dot(X), f * M.dot(X)
    R = AX - MX * r.values[None, :]
    rn = numpy.sqrt((R * R).sum(axis=0))
    xm = numpy.sqrt((X * MX).sum(axis=0))
    width = numpy.diff(A.indptr).max() + 2
    rb = width * EPS * (numpy.abs(A).dot(numpy.abs(X))
                        + numpy.abs(M).dot(numpy.abs(X))
                        * numpy.abs(r.values)[None, :])
    _report('residuals reported against recomputed',
            numpy.abs(rn - r.residuals).max(),
            2.0 * numpy.sqrt((rb * rb).sum(axis=0)).max())
    radius = rn / (numpy.sqrt(lmin) * xm) + 1e3 * EPS * abs(want[k - 1])
    picks = eref.match_once(r.values, want, radius)
    print('reference %s\nradius %s' % (want[:k], radius))
    assert picks == list(range(k)), picks
    _report('largest |lambda - reference| / radius',
            (numpy.abs(r.values - want[:k]) / radius).max(), 1.0)
    if which == 'neumann':
        _report('lambda_0 of the pure Neumann problem', abs(r.values[0]),
                radius[0])
    G = X.T.dot(MX)
    bound = (n + 32) * EPS * numpy.abs(X).T.dot(
        numpy.abs(M).dot(numpy.abs(X))).max()
    _report('X^T M X - I', numpy.abs(G - numpy.eye(k)).max(), bound)
    # rayleigh() agrees with the value to the residual's order
    _report('rayleigh(mode 0)', abs(E.rayleigh(r.modes[0]) - r.values[0]),
            radius[0] + bound * abs(want[k - 1]))
    # the same call twice: the same bits
    r2 = E.solve(k, rtol=1e-9, maxit=400, preconditioner=preconditioner)
    assert numpy.array_equal(r.values.view(numpy.int64),
                             r2.values.view(numpy.int64))
    assert r2.iterations == r.iterations
    for u, w in zip(r.modes, r2.modes):
        assert torch.equal(u.data, w.data)


def test_not_converged(hip):
    a, m, bcs, V = _problem('dirichlet-p1')
    E = fem.Eigenmodes(a, m, bcs)
    with pytest.raises(_hip.NotConverged):
        E.solve(6, maxit=1)
    r = E.solve(6, maxit=1, error_on_nonconvergence=False)
    assert r.iterations == 1 and not r.converged.any()
    assert numpy.isfinite(r.values).all() and numpy.isfinite(r.residuals).all()
    print('maxit 1: values %s residuals %s' % (r.values, r.residuals))


def test_from_matrices_initial_and_eigensolve(hip):
    a, m, bcs, V = _problem('dirichlet-p1')
    A, M, isbc, lmin, want, _ = _reference('dirichlet-p1', 6)
    r = fem.eigensolve(a, m, bcs, k=2, rtol=1e-9)
    E = fem.Eigenmodes.from_matrices(fem.assemble(a), ops.assemble_mass(V),
                                     isbc)
    r2 = E.solve(2, rtol=1e-9, initial=r.modes)
    print('restart from the modes: %d iterations (cold: %d)'
          % (r2.iterations, r.iterations))
    assert r2.iterations < r.iterations
    radius = r2.residuals / numpy.sqrt(lmin) + 1e3 * EPS * want[1]
    assert eref.match_once(r2.values, want, radius) == [0, 1]
    with pytest.raises(ValueError):
        E.solve(2, preconditioner='amg')
    with pytest.raises(ValueError):
        E.solve(40)
