# -*- coding: utf-8 -*-
'''
fem.Eigenmodes without a GPU: the dense Rayleigh-Ritz step against
scipy.linalg.eigh, its fallback for a numerically singular Gram matrix, the
LOBPCG loop on the numpy backend against eigen_reference (scipy's direct
solvers on the eliminated matrices) and the analytic spectrum, the argument
checks, and the bindings.

Bounds.  rayleigh_ritz on an s x s pair: the eigenvalues of the scaled
pencil carry s eps cond(GM) |theta|_max from the Cholesky reduction (Davies,
Higham, Tisseur 2001); the pairs here have cond(GM) <= 1e3, and the bound is
taken with the factor 50 of test_snapshots_host.py's host algebra (C_HOST =
5, times the 10 of the two triangular solves).  The loop: a Ritz value with
residual r lies within |r|_2 / (sqrt(lambda_min(M)) |x|_M) of an eigenvalue
(Krylov-Weinstein), as the GPU tests use it.
'''
import numpy
import pytest
import scipy.linalg

from flow_amd import _hip, fem
from flow_amd.fem import eigen

import bilinear_reference as bref
import eigen_reference as eref

EPS = numpy.finfo(float).eps


def _report(what, err, bound):
    print('%s: error %.2e  bound %.2e' % (what, err, bound))
    assert numpy.isfinite(err) and err <= bound


def _spd_pair(s, seed):
    rng = numpy.random.RandomState(seed)
    Q, _ = numpy.linalg.qr(rng.standard_normal((s, s)))
    GM = (Q * numpy.logspace(0, 3, s)).dot(Q.T)
    B = rng.standard_normal((s, s))
    GA = B + B.T
    return GA, GM


@pytest.mark.parametrize('s', [1, 5, 24, 96])
def test_rayleigh_ritz_against_eigh(s):
    GA, GM = _spd_pair(s, s)
    theta, C = eigen.rayleigh_ritz(GA, GM)
    want = scipy.linalg.eigh(0.5 * (GA + GA.T), 0.5 * (GM + GM.T),
                             eigvals_only=True)
    assert theta.shape == (s,) and C.shape == (s, s)
    assert (numpy.diff(theta) >= 0.0).all()
    scale = numpy.abs(want).max()
    bound = 50 * s * EPS * 1.0e3 * scale
    _report('s %d eigenvalues' % s, numpy.abs(theta - want).max(), bound)
    _report('s %d C^T GM C - I' % s,
            numpy.abs(C.T.dot(GM).dot(C) - numpy.eye(s)).max(),
            50 * s * EPS * 1.0e3)
    _report('s %d C^T GA C - diag' % s,
            numpy.abs(C.T.dot(GA).dot(C) - numpy.diag(theta)).max(), bound)


def test_rayleigh_ritz_unsymmetric_input_is_symmetrised():
    GA, GM = _spd_pair(6, 3)
    E = numpy.triu(numpy.full((6, 6), 1e-13), 1)
    t0, _ = eigen.rayleigh_ritz(GA, GM)
    t1, _ = eigen.rayleigh_ritz(GA + E - E.T, GM + E - E.T)
    assert numpy.array_equal(t0, t1)


def test_rayleigh_ritz_singular_gram_drops_a_direction():
    '''A duplicated column makes GM singular: the Ritz pairs are those of the
    span, one fewer.'''
    rng = numpy.random.RandomState(5)
    n, s = 40, 6
    S = rng.standard_normal((n, s))
    A = numpy.diag(numpy.arange(1.0, n + 1))
    S2 = numpy.concatenate([S, S[:, 2:3]], axis=1)
    want, _ = eigen.rayleigh_ritz(S.T.dot(A).dot(S), S.T.dot(S))
    theta, C = eigen.rayleigh_ritz(S2.T.dot(A).dot(S2), S2.T.dot(S2))
    assert theta.shape == (s,) and C.shape == (s + 1, s)
    bound = 50 * (s + 1) * EPS * numpy.linalg.cond(S.T.dot(S)) * want.max()
    _report('duplicated column: Ritz values', numpy.abs(theta - want).max(),
            bound)
    X = S2.dot(C)
    _report('duplicated column: X^T X - I',
            numpy.abs(X.T.dot(X) - numpy.eye(s)).max(),
            50 * (s + 1) * EPS * numpy.linalg.cond(S.T.dot(S)))
    with pytest.raises(ValueError):
        eigen.rayleigh_ritz(numpy.zeros((3, 3)), numpy.zeros((3, 3)))
    with pytest.raises(ValueError):
        eigen.rayleigh_ritz(numpy.eye(3), numpy.eye(4))


def _laplacian(nx):
    mesh = fem.UnitSquareMesh(nx, nx)
    V = fem.FunctionSpace(mesh, 'P', 1)
    u, v = fem.TrialFunction(V), fem.TestFunction(V)
    A = bref.matrix(fem.inner(fem.grad(u), fem.grad(v)) * fem.dx)
    M = bref.matrix(u * v * fem.dx)
    x = V.layout.dof_coords
    isbc = (numpy.abs(x[:, 0]) < 1e-12) | (numpy.abs(x[:, 0] - 1) < 1e-12) | \
        (numpy.abs(x[:, 1]) < 1e-12) | (numpy.abs(x[:, 1] - 1) < 1e-12)
    return V, A, M, isbc


def _eliminated(A, M, isbc):
    '''symmetric_bc_matrix on the host: identity rows and columns.'''
    import scipy.sparse as sp
    f = sp.diags((~isbc).astype(float))
    d = sp.diags(isbc.astype(float))
    return (f.dot(A).dot(f) + d).tocsr(), (f.dot(M).dot(f) + d).tocsr()


def test_host_loop_dirichlet_laplacian():
    V, A, M, isbc = _laplacian(12)
    k = 6
    Ae, Me = _eliminated(A, M, isbc)
    vals, X, out = eigen.host_eigensolve(Ae, Me, ~isbc, k, rtol=1e-9,
                                         maxit=300)
    assert out.converged[:k].all(), out.residuals
    print('iterations %d' % out.iterations)
    want, Xr = eref.smallest(A, M, isbc, k + 2)
    # the discrete spectrum approximates pi^2 (p^2 + q^2) from above: 2, 5, 5,
    # 8, 10, 10 -- the P1 error on this mesh is below 12 % for these
    exact = numpy.pi ** 2 * numpy.array([2., 5., 5., 8., 10., 10.])
    assert (want[:k] > exact).all() and (want[:k] < 1.12 * exact).all()
    # Krylov-Weinstein per pair
    lmin = eref.mass_lambda_min(M, isbc)
    R = Ae.dot(X) - Me.dot(X) * vals[None, :]
    rn = numpy.sqrt((R * R).sum(axis=0))
    xm = numpy.sqrt((X * Me.dot(X)).sum(axis=0))
    radius = rn / (numpy.sqrt(lmin) * xm)
    _report('reported residuals against recomputed',
            numpy.abs(rn - out.residuals[:k]).max(),
            1e3 * EPS * numpy.abs(Ae).dot(numpy.abs(X)).max())
    picks = eref.match_once(vals, want, radius)
    print('values %s\nreference %s\nradius %s' % (vals, want[:k], radius))
    assert picks == list(range(k))
    assert (X[isbc, :] == 0.0).all()
    _report('X^T M X - I', numpy.abs(X.T.dot(Me.dot(X)) - numpy.eye(k)).max(),
            (X.shape[0] + 32) * EPS
            * numpy.abs(X).T.dot(abs(Me).dot(numpy.abs(X))).max())
    # subspaces of the clusters {0}, {1, 2}, {3}, {4, 5}: the angle is bounded
    # by the residuals over the gap to the rest of the spectrum (Davis-Kahan)
    for idx in ([0], [1, 2], [3], [4, 5]):
        others = numpy.delete(want, idx)
        gap = numpy.abs(others[:, None] - want[idx][None, :]).min()
        bound = numpy.sqrt((radius[idx] ** 2).sum()) / gap * numpy.pi / 2
        _report('cluster %s: principal angle' % idx,
                eref.principal_angle(X[:, idx], Xr[:, idx], Me), bound)


def test_host_loop_neumann_zero_eigenvalue():
    V, A, M, _ = _laplacian(8)
    isbc = numpy.zeros(A.shape[0], dtype=bool)
    vals, X, out = eigen.host_eigensolve(A, M, ~isbc, 3, rtol=1e-9, maxit=300)
    assert out.converged[:3].all()
    want, _ = eref.smallest(A, M, isbc, 3)
    lmin = eref.mass_lambda_min(M, isbc)
    radius = out.residuals[:3] / numpy.sqrt(lmin)       # |x|_M = 1
    print('values %s reference %s radius %s' % (vals, want, radius))
    assert eref.match_once(vals, want, radius + 1e3 * EPS * want.max()) \
        == [0, 1, 2]


def test_argument_checks(monkeypatch):
    mesh = fem.UnitSquareMesh(2, 2)
    V = fem.FunctionSpace(mesh, 'P', 1)
    V2 = fem.FunctionSpace(mesh, 'P', 2)
    u, v = fem.TrialFunction(V), fem.TestFunction(V)
    u2, v2 = fem.TrialFunction(V2), fem.TestFunction(V2)
    a = fem.inner(fem.grad(u), fem.grad(v)) * fem.dx
    # unsymmetric: a convection term
    with pytest.raises(ValueError, match='symmetric'):
        fem.Eigenmodes(a + u.dx(0) * v * fem.dx)
    with pytest.raises(ValueError, match='different spaces'):
        fem.Eigenmodes(a, u2 * v2 * fem.dx)
    with pytest.raises(ValueError, match='rank'):
        fem.Eigenmodes(v * fem.dx)
    # the block
    assert eigen.check_block(6, None, 100) == (6, 2, 8)
    assert eigen.check_block(16, None, 100) == (16, 4, 20)
    assert eigen.check_block(3, 5, 4) == (3, 1, 4)
    with pytest.raises(ValueError, match='at most 32'):
        eigen.check_block(30, 3, 1000)
    with pytest.raises(ValueError, match='at most 32'):
        eigen.check_block(28, None, 1000)
    with pytest.raises(ValueError, match='free dofs'):
        eigen.check_block(10, None, 9)
    with pytest.raises(ValueError):
        eigen.check_block(0, None, 9)
    # strips
    from flow_amd import parallel
    monkeypatch.setattr(parallel, 'active', lambda: True)
    with pytest.raises(NotImplementedError, match='strips'):
        fem.Eigenmodes(a)
    with pytest.raises(NotImplementedError, match='strips'):
        fem.Eigenmodes.from_matrices(None, None)


def test_start_block_is_reproducible_and_masked():
    free = numpy.array([True, False, True, True])
    X = eigen.start_block(4, 2, free)
    assert numpy.array_equal(X, eigen.start_block(4, 2, free))
    assert (X[1] == 0.0).all() and (X[[0, 2, 3]] != 0.0).all()
    Y = eigen.start_block(4, 2, free, [numpy.arange(4.0)])
    assert numpy.array_equal(Y[:, 0], [0.0, 0.0, 2.0, 3.0])
    assert numpy.array_equal(Y[:, 1], X[:, 1])


def test_bindings():
    assert _hip.ABI_VERSION == 30
    for name in ('flow_operator_apply_block', 'flow_block_gram'):
        assert name in _hip.SYMBOLS
    lib = _hip.load_library()
    assert lib.flow_abi_version() == 30
    assert hasattr(lib, 'flow_operator_apply_block')
    assert hasattr(lib, 'flow_block_gram')
    assert fem.Eigenmodes is eigen.Eigenmodes
    assert fem.eigensolve is eigen.eigensolve
