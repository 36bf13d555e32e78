# -*- coding: utf-8 -*-
'''
fem.Eigenmodes on vector spaces on the device (fem.vector_eigenmodes): the
block product of a 2x2-block operator (kind 2) against flow_operator_apply,
whose bits it promises, and the eigensolver against eigen_reference (scipy's
direct solver on the 2N x 2N matrices read back from the device).

Bounds (every test prints its measured error next to its bound, pytest -s),
those of test_eigen_gpu.py:

apply_block      every column bit-equal to flow_operator_apply on that column
                 (torch.equal), the padding of Y and the columns >= m
                 untouched, two calls bit-equal.
eigenvalues      a returned lambda_j lies within |r_j|_2 / (sqrt(lambda_min(
                 M_free)) |x_j|_M) of an eigenvalue (Krylov-Weinstein), r_j
                 recomputed on the host from the matrices read back; on top,
                 the reference's own error: 1e3 eps lambda_k (eigh).  The k
                 reference values are each matched once.
X^T M X - I      (n + 32) eps | |X|^T |M| |X| |, n = 2N.
residuals        reported against recomputed: (nnz per row + 2) eps (|A| |x| +
                 |lambda| |M| |x|) per entry, in the 2-norm, times 2.
vector Laplacian inner(grad u, grad v) is the scalar stiffness matrix on each
                 component: every scalar eigenvalue twice.  Two solves of this
                 package are compared, each value within its own radius
                 (reported residual / sqrt(lambda_min(M_free)), the modes being
                 M-orthonormal, plus 1e3 eps lambda_k for the rounding of the
                 Rayleigh quotients) of an eigenvalue: the sum of the two.
rigid-body modes the interpolants of (1, 0), (0, 1), (-y, x) span the kernel
                 of the free body's A exactly; the computed invariant subspace
                 of the three smallest values is within max_j |r_j|_2 /
                 (sqrt(lambda_min(M)) lambda_3) of it (Davis-Kahan, the gap
                 being lambda_3), in the M-norm, plus 1e3 eps.
'''
import ctypes
import functools

import numpy
import pytest
import torch

from flow_amd import _hip, device, fem
from flow_amd.fem import ops, inner, grad, dot, sym, tr, Identity, dx

import eigen_reference as eref

pytestmark = pytest.mark.gpu

EPS = numpy.finfo(float).eps
MC2 = 2                      # kBlockMC2 of csrc/eigen_kernels.hip
MU, LAM = 1.0, 1.25


@pytest.fixture(autouse=True)
def _switches_on():
    with fem.vector_arguments(True), fem.vector_eigenmodes(True):
        yield


def _report(what, err, bound):
    print('%s: error %.2e  bound %.2e' % (what, err, bound))
    assert numpy.isfinite(err) and err <= bound


def _eps(w):
    return sym(grad(w))


def _sigma(w):
    return 2.0 * MU * _eps(w) + LAM * tr(_eps(w)) * Identity(2)


def _elasticity(W):
    u, v = fem.TrialFunction(W), fem.TestFunction(W)
    return inner(_sigma(u), _eps(v)) * dx


# -- 1. apply_block on kind 2 -------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _matrix(which):
    '''Four distinct planes, A_xy != A_yx^T.'''
    if which == 'p1-tiny':
        W = fem.VectorFunctionSpace(fem.UnitSquareMesh(1, 1), 'P', 1)
    elif which == 'p1':
        W = fem.VectorFunctionSpace(fem.UnitSquareMesh(20, 20), 'P', 1)
    elif which == 'p2':
        W = fem.VectorFunctionSpace(fem.UnitSquareMesh(20, 20), 'P', 2)
    else:
        W = fem.VectorFunctionSpace(fem.karman_channel_graded(lcar=1.0e-2),
                                    'P', 2)
    u, v = fem.TrialFunction(W), fem.TestFunction(W)
    A = fem.assemble(inner(_sigma(u), _eps(v)) * dx + u[0] * v[1] * dx
                     + 3 * u[1] * v[0] * dx)
    return W, A


@pytest.mark.parametrize('chunk', [0, 2, 4])
@pytest.mark.parametrize('which', ['p1-tiny', 'p1', 'p2', 'graded'])
def test_apply_block_bits(hip, which, chunk):
    W, A = _matrix(which)
    assert A.kind == 2
    N = W.N
    n = 2 * N
    assert A.size == n
    if which == 'p1-tiny':
        assert N == 4
    if which == 'p2':
        assert N == 1681 and A.operator().nblocks > 1
    mmax = 2 * 4 + 1
    ldx, ldy = (n + 3) & ~1, (n + 5) & ~1
    rng = numpy.random.RandomState(N % 997)
    X = numpy.full((mmax, ldx), numpy.nan)
    X[:, :n] = rng.uniform(-1.0, 1.0, size=(mmax, n))
    Xd = device.to_device(X.reshape(-1))
    mc = chunk or MC2
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
        Zd = device.empty(mmax * ldy)
        Zd.fill_(-7.0)
        A.apply_block(Xd, ldx, m, Zd, ldy, chunk=chunk)
        assert torch.equal(Yd, Zd)
    print('%s (N %d, %d row blocks) chunk %d: all columns bit-equal'
          % (which, N, A.operator().nblocks, mc))


# -- 2. refusals ---------------------------------------------------------------------------
def test_apply_block_refusals(hip):
    W, A = _matrix('p1')
    n = 2 * W.N
    ld = n
    assert ld % 2 == 0
    X = device.zeros(4 * ld + 2)
    Y = device.zeros(4 * ld + 2)
    M1 = ops.Matrix(W.layout, 1)         # (its zero fill is a launch)
    op = ctypes.byref(A.operator())
    st = _hip.stream()
    before = _hip.launch_count()

    def call(m, x, ldx, y, ldy, mc=0):
        return hip.flow_operator_apply_block_chunk(
            op, m, _hip.f64(x), ldx, _hip.f64(y), ldy, mc, st)
    assert call(2, X, ld - 2, Y, ld) == 2           # ldx < 2N
    assert call(2, X, (W.N + 3) & ~1, Y, ld) == 2   # N <= ldx < 2N, even
    assert call(2, X, ld + 1, Y, ld + 2) == 2       # odd ldx
    assert call(2, X[1:], ld, Y, ld) == 2           # misaligned X
    assert call(2, X, ld, Y[1:], ld) == 2           # misaligned Y
    assert call(2, X, ld, X[ld:], ld) == 2          # Y overlaps X
    assert call(2, X, ld, Y, ld, 3) == 2            # chunk
    assert call(2, X, ld, Y, ld, 8) == 2            # chunk 8: no LDS for kind 2
    with pytest.raises(ValueError):
        A.apply_block(X, ld, 2, Y, ld, chunk=8)
    with pytest.raises(ValueError):
        M1.apply_block(X, ld, 1, Y, ld)
    assert hip.flow_operator_apply_block(
        ctypes.byref(M1.operator()), 1, _hip.f64(X), ld, _hip.f64(Y), ld,
        st) == 2
    assert call(0, X, ld, Y, ld) == 0               # nothing to do
    assert _hip.launch_count() == before


# -- 3. the eigensolver against the reference ---------------------------------------------
def _left(p, on):
    return on and p[0] < 1e-10


def _bottom(p, on):
    return on and p[1] < 1e-10


def _problem(which):
    '''(a, m, bcs, W) of the named problem.'''
    if which == 'clamped-p2':
        W = fem.VectorFunctionSpace(fem.UnitSquareMesh(8, 8), 'P', 2)
    else:
        W = fem.VectorFunctionSpace(fem.UnitSquareMesh(12, 12), 'P', 1)
    a = _elasticity(W)
    if which == 'roller':
        u, v = fem.TrialFunction(W), fem.TestFunction(W)
        bcs = [fem.DirichletBC(W.sub(1), 0.0, _bottom),
               fem.DirichletBC(W.sub(0), 0.0, _left)]
        return a, 2.0 * dot(u, v) * dx, bcs, W
    return a, None, [fem.DirichletBC(W, (0.0, 0.0), _left)], W


def _host_matrices(a, m, bcs, W):
    if m is None:
        m = dot(fem.TrialFunction(W), fem.TestFunction(W)) * dx
    A = fem.assemble(a).to_scipy()
    M = fem.assemble(m).to_scipy()
    isbc = numpy.zeros(W.size(), dtype=bool)
    _, _, mask = ops._scalar_bcs(bcs, W)
    if mask is not None:
        isbc = device.to_host(mask).numpy().astype(bool)
    return A, M, isbc


@functools.lru_cache(maxsize=None)
def _reference(which, k):
    '''The unconstrained host matrices as the device assembled them, the
    Dirichlet mask (2N), lambda_min(M_free) and the reference eigenvalues.'''
    A, M, isbc = _host_matrices(*_problem(which))
    want, _ = eref.smallest(A, M, isbc, k + 2)
    return A, M, isbc, eref.mass_lambda_min(M, isbc), want


def _check(E, r, k, A, M, isbc, lmin, want):
    '''The checks of test_eigen_gpu.py on a result of 2N-entry modes; returns
    (X, residual norms recomputed, radius).'''
    n = A.shape[0]
    assert r.converged.all() and len(r.modes) == k
    assert (numpy.diff(r.values) >= 0.0).all()
    for u in r.modes:
        assert isinstance(u, fem.Function) and u.data.numel() == n
        if E.V is not None:
            assert u.function_space() is E.V
    X = numpy.stack([device.to_host(u.data).numpy() for u in r.modes], axis=1)
    assert X.shape == (n, k)
    assert (X[isbc, :] == 0.0).all()
    for j in range(k):
        i = int(numpy.argmax(numpy.abs(X[:, j])))
        assert X[i, j] > 0.0
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
    G = X.T.dot(MX)
    bound = (n + 32) * EPS * numpy.abs(X).T.dot(
        numpy.abs(M).dot(numpy.abs(X))).max()
    _report('X^T M X - I', numpy.abs(G - numpy.eye(k)).max(), bound)
    _report('rayleigh(mode %d)' % (k - 1),
            abs(E.rayleigh(r.modes[k - 1]) - r.values[k - 1]),
            radius[k - 1] + bound * abs(want[k - 1]))
    return X, rn, radius


CASES = [('clamped-p1', 4), ('clamped-p1', 6), ('clamped-p2', 4),
         ('clamped-p2', 6), ('roller', 4)]


@pytest.mark.parametrize('preconditioner', ['jacobi', 'two_level'])
@pytest.mark.parametrize('which,k', CASES)
def test_eigenmodes_against_reference(hip, which, k, preconditioner):
    a, m, bcs, W = _problem(which)
    A, M, isbc, lmin, want = _reference(which, k)
    assert isbc.shape == (2 * W.N,) and isbc.any()
    if which == 'roller':
        # the two components are constrained on different sides
        assert (isbc[:W.N] != isbc[W.N:]).any()
    E = fem.Eigenmodes(a, m, bcs)
    assert E.A.kind == 2 and E.M.kind == 2
    assert numpy.array_equal(E.isbc, isbc) and E.free.shape == (2 * W.N,)
    r = E.solve(k, rtol=1e-9, maxit=600, preconditioner=preconditioner)
    print('%s k %d %s: %d iterations, values %s'
          % (which, k, preconditioner, r.iterations, r.values))
    _check(E, r, k, A, M, isbc, lmin, want)


# -- 4. the vector Laplacian ---------------------------------------------------------------
def test_vector_laplacian_doubles_the_scalar_spectrum(hip):
    mesh = fem.UnitSquareMesh(10, 10)
    V = fem.FunctionSpace(mesh, 'P', 1)
    W = fem.VectorFunctionSpace(mesh, 'P', 1)
    us, vs = fem.TrialFunction(V), fem.TestFunction(V)
    u, v = fem.TrialFunction(W), fem.TestFunction(W)
    k = 6
    rs = fem.Eigenmodes(inner(grad(us), grad(vs)) * dx, None,
                        fem.DirichletBC(V, 0.0, 'on_boundary')) \
        .solve(k // 2, rtol=1e-9, maxit=400)
    bc = fem.DirichletBC(W, (0.0, 0.0), 'on_boundary')
    rv = fem.Eigenmodes(inner(grad(u), grad(v)) * dx, None, bc) \
        .solve(k, rtol=1e-9, maxit=400)
    Ms = fem.assemble(us * vs * dx).to_scipy()
    _, _, mask = ops._scalar_bcs([fem.DirichletBC(V, 0.0, 'on_boundary')], V)
    lmin = eref.mass_lambda_min(
        Ms, device.to_host(mask).numpy().astype(bool))
    scale = 1e3 * EPS * rv.values[-1]
    rad_s = rs.residuals / numpy.sqrt(lmin) + scale
    rad_v = rv.residuals / numpy.sqrt(lmin) + scale
    print('scalar %s\nvector %s\nradii %s %s'
          % (rs.values, rv.values, rad_s, rad_v))
    assert rs.converged.all() and rv.converged.all()
    twice = numpy.repeat(rs.values, 2)
    _report('largest |vector - scalar twice| / (sum of radii)',
            (numpy.abs(rv.values - twice)
             / (rad_v + numpy.repeat(rad_s, 2))).max(), 1.0)


# -- 5. the free body ----------------------------------------------------------------------
def test_free_body_rigid_modes(hip):
    W = fem.VectorFunctionSpace(fem.UnitSquareMesh(10, 10), 'P', 1)
    a = _elasticity(W)
    A, M, isbc = _host_matrices(a, None, None, W)
    assert not isbc.any()
    k = 4
    want, _ = eref.smallest(A, M, isbc, k + 2)
    lmin = eref.mass_lambda_min(M, isbc)
    E = fem.Eigenmodes(a)
    r = E.solve(k, rtol=1e-9, maxit=600, preconditioner='jacobi')
    print('free body: %d iterations, values %s' % (r.iterations, r.values))
    X, rn, radius = _check(E, r, k, A, M, isbc, lmin, want)
    _report('largest |lambda_0..2| / radius',
            (numpy.abs(r.values[:3]) / radius[:3]).max(), 1.0)
    assert r.values[3] > radius[3]
    x = W.layout.dof_coords
    one, zero = numpy.ones(W.N), numpy.zeros(W.N)
    X3 = X[:, :3]
    defect = rn[:3].max() / (numpy.sqrt(lmin) * r.values[3]) + 1e3 * EPS
    for name, z in (('(1, 0)', numpy.concatenate([one, zero])),
                    ('(0, 1)', numpy.concatenate([zero, one])),
                    ('(-y, x)', numpy.concatenate([-x[:, 1], x[:, 0]]))):
        d = z - X3.dot(X3.T.dot(M.dot(z)))
        zm = numpy.sqrt(z.dot(M.dot(z)))
        _report('%s outside the first three modes, M-norm' % name,
                numpy.sqrt(max(d.dot(M.dot(d)), 0.0)), defect * zm)


# -- 6. determinism, from_matrices ---------------------------------------------------------
def test_same_bits_and_from_matrices(hip):
    a, m, bcs, W = _problem('clamped-p1')
    A, M, isbc, lmin, want = _reference('clamped-p1', 4)
    E = fem.Eigenmodes(a, m, bcs)
    r = E.solve(4, rtol=1e-9, maxit=600)
    r2 = E.solve(4, rtol=1e-9, maxit=600)
    assert numpy.array_equal(r.values.view(numpy.int64),
                             r2.values.view(numpy.int64))
    assert r2.iterations == r.iterations
    for u, w in zip(r.modes, r2.modes):
        assert torch.equal(u.data, w.data)
    A2 = fem.assemble(a)
    M2 = fem.assemble(dot(fem.TrialFunction(W), fem.TestFunction(W)) * dx)
    assert A2.kind == 2 and M2.kind == 2
    F = fem.Eigenmodes.from_matrices(A2, M2, isbc)
    loose = E.solve(4, rtol=1e-5, maxit=600)
    cold = F.solve(4, rtol=1e-9, maxit=600)
    warm = F.solve(4, rtol=1e-9, maxit=600, initial=loose.modes)
    print('from_matrices: cold %d iterations, from the modes of a solve to '
          '1e-5 (%d iterations): %d' % (cold.iterations, loose.iterations,
                                        warm.iterations))
    assert warm.iterations < cold.iterations
    assert numpy.array_equal(cold.values.view(numpy.int64),
                             r.values.view(numpy.int64))
    radius = warm.residuals / numpy.sqrt(lmin) + 1e3 * EPS * want[3]
    assert eref.match_once(warm.values, want, radius) == [0, 1, 2, 3]
    # modes without a space are device tensors of 2N entries
    assert warm.modes[0].numel() == 2 * W.N
    V = fem.FunctionSpace(W.mesh(), 'P', 1)
    with pytest.raises(ValueError):
        fem.Eigenmodes.from_matrices(A2, ops.assemble_mass(V), isbc)
    with pytest.raises(ValueError):
        fem.Eigenmodes.from_matrices(ops.assemble_stiffness(V), M2)
    with pytest.raises(ValueError):
        fem.Eigenmodes.from_matrices(A2, M2, isbc[:W.N])
    with pytest.raises(ValueError):
        F.solve(4, initial=[fem.Function(V)])
