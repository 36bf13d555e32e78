# -*- coding: utf-8 -*-
'''
fem.Eigenmodes on vector spaces (eigen.vector_eigenmodes) without a GPU: the
switch, the form checks with it off and on, the LOBPCG loop on the numpy
backend for 2N x 2N block matrices of P1 elasticity -- a body clamped on one
edge and a free body with its three rigid-body modes -- against
eigen_reference (scipy.linalg.eigh on the free dofs), and the bindings.

The matrices are built here in numpy from constant-strain triangles
(component-blocked: x then y), not by the package.

Bound.  A Ritz value with residual r lies within |r|_2 / (sqrt(lambda_min(M))
|x|_M) of an eigenvalue (Krylov-Weinstein), as test_eigen_host.py uses it.
'''
import numpy
import pytest
import scipy.sparse as sp

from flow_amd import _hip, fem
from flow_amd.fem import eigen, forms

import eigen_reference as eref

EPS = numpy.finfo(float).eps
MU, LAM = 1.0, 1.25


@pytest.fixture
def on():
    with forms.vector_arguments(True):
        yield


def _spaces():
    mesh = fem.UnitSquareMesh(3, 3)
    return mesh, fem.VectorFunctionSpace(mesh, 'P', 1)


def _forms(W):
    u, v = fem.TrialFunction(W), fem.TestFunction(W)
    eps = lambda w: fem.sym(fem.grad(w))                    # noqa: E731
    a = (2 * MU * fem.inner(eps(u), eps(v))
         + LAM * fem.div(u) * fem.div(v)) * fem.dx
    return u, v, a, fem.dot(u, v) * fem.dx


# -- the switch ---------------------------------------------------------------------------
def test_switch_off(on):
    mesh, W = _spaces()
    u, v, a, m = _forms(W)
    assert fem.vector_eigenmodes.enabled is False
    with pytest.raises(NotImplementedError, match='vector space'):
        eigen._check_forms(a, m, False)
    with pytest.raises(NotImplementedError, match='vector_eigenmodes'):
        eigen._check_forms(a, None, False)
    with fem.vector_eigenmodes(True) as s:
        assert s.previous is False and fem.vector_eigenmodes.enabled is True
        with fem.vector_eigenmodes(False):
            assert fem.vector_eigenmodes.enabled is False
        assert fem.vector_eigenmodes.enabled is True
    assert fem.vector_eigenmodes.enabled is False
    # the other switches are their own
    assert forms.vector_arguments.enabled is True
    assert forms.vector_derivatives.enabled is False


def test_switch_on(on):
    mesh, W = _spaces()
    u, v, a, m = _forms(W)
    with fem.vector_eigenmodes(True):
        assert eigen._check_forms(a, m, False) is W
        assert eigen._check_forms(a, None, False) is W
        # an unsymmetric block form
        bad = a + u[0] * v[1] * fem.dx
        with pytest.raises(ValueError, match='symmetric'):
            eigen._check_forms(bad, m, False)
        assert eigen._check_forms(bad, m, True) is W
        with pytest.raises(ValueError, match='rank'):
            eigen._check_forms(fem.dot(fem.Constant((1.0, 0.0)), v) * fem.dx,
                               None, False)
        # a space of another degree
        W2 = fem.VectorFunctionSpace(mesh, 'P', 2)
        m2 = fem.dot(fem.TrialFunction(W2), fem.TestFunction(W2)) * fem.dx
        with pytest.raises(ValueError, match='different spaces'):
            eigen._check_forms(a, m2, False)
        # component views and mixed spaces carry no arguments with the switch
        # on either, so a form on them cannot be written
        with pytest.raises(NotImplementedError):
            fem.TrialFunction(W.sub(0))
        P = fem.FiniteElement('P', 'triangle', 1)
        mixed = fem.FunctionSpace(mesh, fem.VectorElement('P', 'triangle', 2) * P)
        with pytest.raises(NotImplementedError):
            fem.TrialFunction(mixed)
    assert fem.vector_eigenmodes.enabled is False


# -- the loop on block matrices -----------------------------------------------------------
def _elasticity(nx):
    '''(A, M, coords) of P1 elasticity on UnitSquareMesh(nx, nx), 2N x 2N,
    component-blocked, from constant-strain triangles.'''
    V = fem.FunctionSpace(fem.UnitSquareMesh(nx, nx), 'P', 1)
    x = V.layout.dof_coords
    cd = numpy.asarray(V.layout.cell_dofs)
    N = V.N
    D = numpy.array([[LAM + 2 * MU, LAM, 0.0], [LAM, LAM + 2 * MU, 0.0],
                     [0.0, 0.0, MU]])
    Me = (numpy.ones((3, 3)) + numpy.eye(3)) / 12.0
    rows, cols, va, vm = [], [], [], []
    for tri in cd:
        p = x[tri]
        J = numpy.array([p[1] - p[0], p[2] - p[0]]).T
        area = 0.5 * abs(numpy.linalg.det(J))
        # gradients of the barycentric functions: rows of G
        G = numpy.concatenate([[-1.0, -1.0], [1.0, 0.0], [0.0, 1.0]]) \
            .reshape(3, 2).dot(numpy.linalg.inv(J))
        B = numpy.zeros((3, 6))
        B[0, :3] = G[:, 0]
        B[1, 3:] = G[:, 1]
        B[2, :3] = G[:, 1]
        B[2, 3:] = G[:, 0]
        Ke = area * B.T.dot(D).dot(B)
        Mk = numpy.zeros((6, 6))
        Mk[:3, :3] = Mk[3:, 3:] = area * Me
        dofs = numpy.concatenate([tri, tri + N])
        rows.append(numpy.repeat(dofs, 6))
        cols.append(numpy.tile(dofs, 6))
        va.append(Ke.ravel())
        vm.append(Mk.ravel())
    rows, cols = numpy.concatenate(rows), numpy.concatenate(cols)
    shape = (2 * N, 2 * N)
    A = sp.coo_matrix((numpy.concatenate(va), (rows, cols)), shape=shape).tocsr()
    M = sp.coo_matrix((numpy.concatenate(vm), (rows, cols)), shape=shape).tocsr()
    return A, M, x


def _eliminated(A, M, isbc):
    f = sp.diags((~isbc).astype(float))
    d = sp.diags(isbc.astype(float))
    return (f.dot(A).dot(f) + d).tocsr(), (f.dot(M).dot(f) + d).tocsr()


def _radius(Ae, Me, M, isbc, vals, X):
    R = Ae.dot(X) - Me.dot(X) * vals[None, :]
    rn = numpy.sqrt((R * R).sum(axis=0))
    xm = numpy.sqrt((X * Me.dot(X)).sum(axis=0))
    return rn / (numpy.sqrt(eref.mass_lambda_min(M, isbc)) * xm)


def test_host_loop_clamped_elasticity():
    A, M, x = _elasticity(6)
    N = len(x)
    clamp = numpy.abs(x[:, 0]) < 1e-12
    isbc = numpy.concatenate([clamp, clamp])
    k = 4
    Ae, Me = _eliminated(A, M, isbc)
    vals, X, out = eigen.host_eigensolve(Ae, Me, ~isbc, k, rtol=1e-9,
                                         maxit=400)
    assert out.converged[:k].all(), out.residuals
    assert X.shape == (2 * N, k) and (X[isbc, :] == 0.0).all()
    want, _ = eref.smallest(A, M, isbc, k + 2)
    radius = _radius(Ae, Me, M, isbc, vals, X)
    print('iterations %d\nvalues %s\nreference %s\nradius %s'
          % (out.iterations, vals, want[:k], radius))
    assert (want[:k] > 0.0).all()
    assert eref.match_once(vals, want, radius) == list(range(k))
    print('largest |lambda - reference| / radius: %.2e'
          % (numpy.abs(vals - want[:k]) / radius).max())


def test_host_loop_free_body_rigid_modes():
    A, M, x = _elasticity(6)
    isbc = numpy.zeros(A.shape[0], dtype=bool)
    k = 4
    vals, X, out = eigen.host_eigensolve(A, M, ~isbc, k, rtol=1e-9, maxit=400)
    assert out.converged[:k].all(), out.residuals
    radius = _radius(A, M, M, isbc, vals, X)
    print('iterations %d\nvalues %s\nradius %s' % (out.iterations, vals, radius))
    assert (numpy.abs(vals[:3]) <= radius[:3]).all()
    assert vals[3] > radius[3]


# -- bindings -------------------------------------------------------------------------------
def test_bindings():
    assert _hip.ABI_VERSION == 30
    assert _hip.load_library().flow_abi_version() == 30
    assert 'flow_operator_apply_block_chunk' in _hip.SYMBOLS
    assert fem.vector_eigenmodes is eigen.vector_eigenmodes
    assert issubclass(fem.vector_eigenmodes, forms._Switch)
    assert fem.vector_eigenmodes.enabled is False
