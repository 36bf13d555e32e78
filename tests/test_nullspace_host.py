# -*- coding: utf-8 -*-
'''
fem.VectorSpaceBasis and solve(..., nullspace=ns) without a GPU: the host
models of tests/nullspace_reference.py against each other, the rigid-body
modes, the argument checks that need no device, and flow_deflate's declaration,
binding and refusals.
'''
import ctypes
import os

import numpy
import pytest
import scipy.sparse as sp

from flow_amd import fem
from flow_amd.fem import nullspace

import nullspace_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52


def _random_basis(rng, k, n):
    Q, _ = numpy.linalg.qr(rng.standard_normal((n, k)))
    return numpy.ascontiguousarray(Q.T)


# -- the models ---------------------------------------------------------------------
def test_deflation_models_agree():
    rng = numpy.random.RandomState(0)
    for n, k in ((1, 1), (7, 3), (300, 8)):
        Z = _random_basis(rng, k, n) if n >= k else numpy.ones((1, 1))
        x = rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 3, n)
        xl, cl = ref.deflate(Z, x)
        xf, cf = ref.deflate_fsum(Z, x)
        xb, cb = ref.deflate_bound(Z, x)
        # both are far inside the bound of the fp64 chain: fsum rounds c once
        # (eps / 2 |c|) and x once more; longdouble has 11 more bits
        assert (numpy.abs(cf - cl.astype(float)) <= cb).all()
        assert (numpy.abs(xf - xl.astype(float)) <= xb).all()
        # a plain fp64 evaluation obeys the bound as well
        c64 = Z.dot(x)
        x64 = x.copy()
        for j in range(k):
            x64 = x64 - c64[j] * Z[j]
        assert (numpy.abs(c64 - cl.astype(float)) <= cb).all()
        assert (numpy.abs(x64 - xl.astype(float)) <= 2.0 * xb).all()
        # the projection is idempotent to rounding
        again, c2 = ref.deflate(Z, xl.astype(float))
        assert numpy.abs(c2.astype(float)).max() <= 4.0 * cb.max() + 1e-300


def _path_laplacian(n):
    d = numpy.full(n, 2.0)
    d[0] = d[-1] = 1.0
    return sp.diags([-numpy.ones(n - 1), d, -numpy.ones(n - 1)], [-1, 0, 1],
                    format='csr')


def test_bordered_lu_against_the_pseudo_inverse():
    rng = numpy.random.RandomState(1)
    n = 40
    S = _path_laplacian(n)
    Z = numpy.full((1, n), 1.0 / numpy.sqrt(n))
    b = rng.standard_normal(n)
    x, lam, res = ref.bordered_solve(S, Z, b)
    assert res < 1e-13
    want = numpy.linalg.pinv(S.toarray()).dot(b)
    assert numpy.abs(x - want).max() <= 1e-11 * numpy.abs(want).max()
    assert abs(Z.dot(x)[0]) <= 1e-12 * numpy.abs(x).max() * numpy.sqrt(n)
    assert abs(lam[0] - Z.dot(b)[0]) <= 1e-12 * numpy.abs(b).max() * n
    # consistent data: lambda vanishes and S x = b
    bl, _ = ref.deflate(Z, b)
    x2, lam2, _ = ref.bordered_solve(S, Z, bl.astype(float))
    assert abs(lam2[0]) <= 1e-13 * numpy.linalg.norm(b)
    assert numpy.abs(x2 - x).max() <= 1e-12 * numpy.abs(x).max()
    # no basis: the plain LU of a regular matrix
    R = S + sp.identity(n)
    x3, lam3, res3 = ref.bordered_solve(R, numpy.zeros((0, n)), b)
    assert len(lam3) == 0 and res3 < 1e-13
    assert numpy.abs(R.dot(x3) - b).max() <= 1e-13 * numpy.abs(b).max() * n


# -- bases --------------------------------------------------------------------------
def _strain_of_linear_field(W, z):
    '''max |eps(u)| per cell of the vector field with the dofs z of W, from
    the vertex values (a P1 gradient), and how far the edge dofs of a P2
    space are from the mean of their vertices: both vanish iff the P1 / P2
    interpolant is a rigid motion (for a field that is linear).'''
    lay = W.layout
    N = W.N
    pts = lay.dof_coords
    cd = lay.cell_dofs[:, :3]
    worst = 0.0
    for cell in cd:
        X = pts[cell]
        B = numpy.array([X[1] - X[0], X[2] - X[0]])
        G = numpy.zeros((2, 2))
        for a in range(2):
            ua = z[a * N + cell]
            G[a] = numpy.linalg.solve(B, [ua[1] - ua[0], ua[2] - ua[0]])
        worst = max(worst, numpy.abs(0.5 * (G + G.T)).max())
    off = 0.0
    if W.degree == 2:
        # (local edge e of cell_dofs[:, 3 + e]: its coordinates are the mean
        # of two vertices; a linear field takes the mean of their values)
        for cell in lay.cell_dofs:
            for e in range(3, 6):
                for i in range(3):
                    for j in range(i + 1, 3):
                        mid = 0.5 * (pts[cell[i]] + pts[cell[j]])
                        if numpy.abs(mid - pts[cell[e]]).max() < 1e-14:
                            for a in range(2):
                                off = max(off, abs(
                                    z[a * N + cell[e]] - 0.5 * (
                                        z[a * N + cell[i]]
                                        + z[a * N + cell[j]])))
    return worst, off


@pytest.mark.parametrize('degree', [1, 2])
def test_rigid_body_modes(degree):
    mesh = fem.UnitSquareMesh(5, 4)
    W = fem.VectorFunctionSpace(mesh, 'Lagrange', degree)
    ns = fem.rigid_body_modes(W)
    assert ns.dim() == 3 and ns.support == (0, W.size())
    assert ns.is_orthonormal(1e-14)
    Z = ns.host()
    assert numpy.abs(Z.dot(Z.T) - numpy.eye(3)).max() <= 16 * EPS
    for j in range(3):
        strain, off = _strain_of_linear_field(W, Z[j])
        assert strain <= 64 * EPS and off <= 16 * EPS, (j, strain, off)
    # the third one turns: its curl does not vanish
    c = W.layout.dof_coords
    rot = numpy.concatenate([-c[:, 1], c[:, 0]])
    assert abs(Z[2].dot(rot)) > 0.1 * numpy.linalg.norm(rot)
    with pytest.raises(ValueError, match='VectorFunctionSpace'):
        fem.rigid_body_modes(fem.FunctionSpace(mesh, 'Lagrange', 1))


def test_constant_nullspace_and_supports():
    mesh = fem.UnitSquareMesh(4, 3)
    for degree in (1, 2):
        V = fem.FunctionSpace(mesh, 'Lagrange', degree)
        ns = fem.constant_nullspace(V)
        assert ns.dim() == 1 and ns.support == (0, V.N)
        assert ns.is_orthonormal(1e-14)
        assert numpy.ptp(ns.host()) == 0.0
    WP = fem.FunctionSpace(
        mesh, fem.VectorElement('Lagrange', 'triangle', 2)
        * fem.FiniteElement('Lagrange', 'triangle', 1))
    W, P = WP.taylor_hood()
    ns = fem.constant_nullspace(WP)
    assert ns.support == (W.size(), P.N) and ns.space is WP
    assert ns.is_orthonormal(1e-14)
    # the same basis handed over as a full-length vector: the support is found
    full = numpy.zeros(WP.size())
    full[W.size():] = 1.0 / numpy.sqrt(P.N)
    same = fem.VectorSpaceBasis([full])
    assert same.support == ns.support
    assert numpy.array_equal(same.host(), ns.host())
    assert same.length == WP.size() and ns.length is None
    with pytest.raises(ValueError, match='scalar space'):
        fem.constant_nullspace(fem.VectorFunctionSpace(mesh, 'Lagrange', 1))


def test_orthonormalize_on_the_host():
    rng = numpy.random.RandomState(2)
    n = 257
    raw = rng.standard_normal((4, n)) + 3.0      # far from orthogonal
    ns = fem.VectorSpaceBasis(list(raw))
    assert not ns.is_orthonormal(1e-6)
    assert ns.orthonormalize() is ns
    assert ns.is_orthonormal(1e-14)
    # the same span, vector by vector (Gram-Schmidt keeps the flags)
    Z = ns.host()
    for j in range(4):
        coef = numpy.linalg.lstsq(raw[:j + 1].T, Z[j], rcond=None)[0]
        assert numpy.abs(raw[:j + 1].T.dot(coef) - Z[j]).max() < 1e-12
    with pytest.raises(ValueError, match='depends linearly'):
        fem.VectorSpaceBasis([raw[0], raw[1], raw[0] + raw[1]]
                             ).orthonormalize()
    with pytest.raises(ValueError, match='1 to 8'):
        fem.VectorSpaceBasis(list(rng.standard_normal((9, 12))))
    with pytest.raises(ValueError, match='1 to 8'):
        fem.VectorSpaceBasis([])
    with pytest.raises(ValueError, match='differ in length'):
        fem.VectorSpaceBasis([numpy.ones(4), numpy.ones(5)])
    with pytest.raises(ValueError, match='support'):
        fem.VectorSpaceBasis([numpy.ones(4)], support=(2, 5))
    with pytest.raises(ValueError, match='all zero'):
        fem.VectorSpaceBasis([numpy.zeros(4)])


# -- the checks of nullspace= that need no device -------------------------------------
def test_validate():
    mesh = fem.UnitSquareMesh(4, 3)
    V = fem.FunctionSpace(mesh, 'Lagrange', 1)
    V2 = fem.FunctionSpace(mesh, 'Lagrange', 2)
    ns = fem.constant_nullspace(V)
    nullspace.validate(ns, V, None)
    nullspace.validate(ns, V, numpy.zeros(0, dtype=numpy.int32))
    with pytest.raises(TypeError, match='VectorSpaceBasis'):
        nullspace.validate([numpy.ones(V.N)], V, None)
    with pytest.raises(ValueError, match='not orthonormal'):
        nullspace.validate(fem.VectorSpaceBasis([numpy.ones(V.N)]), V, None)
    with pytest.raises(ValueError, match='another space'):
        nullspace.validate(ns, V2, None)
    with pytest.raises(ValueError, match='wrong length'):
        nullspace.validate(
            fem.VectorSpaceBasis([numpy.full(V.N, V.N ** -0.5)]), V2, None)
    with pytest.raises(ValueError, match='wrong length'):
        nullspace.validate(
            fem.VectorSpaceBasis([numpy.full(V2.N, V2.N ** -0.5)],
                                 support=(2, V2.N)), V, None)
    with pytest.raises(ValueError, match='Dirichlet dof'):
        nullspace.validate(ns, V, numpy.array([3], dtype=numpy.int32))
    # a basis that vanishes on the Dirichlet dofs passes
    z = numpy.ones(V.N)
    z[3] = 0.0
    ok = fem.VectorSpaceBasis([z / numpy.linalg.norm(z)])
    nullspace.validate(ok, V, numpy.array([3], dtype=numpy.int32))
    # on a Taylor-Hood space only dofs inside the support count
    WP = fem.FunctionSpace(
        mesh, fem.VectorElement('Lagrange', 'triangle', 2)
        * fem.FiniteElement('Lagrange', 'triangle', 1))
    W, P = WP.taylor_hood()
    nsp = fem.constant_nullspace(WP)
    nullspace.validate(nsp, WP, numpy.arange(W.size(), dtype=numpy.int32))
    with pytest.raises(ValueError, match='Dirichlet dof'):
        nullspace.validate(nsp, WP, numpy.array([W.size() + 1]))
    with pytest.raises(ValueError, match='another space'):
        nullspace.validate(ns, WP, None)


def test_solve_takes_the_keyword():
    import inspect
    from flow_amd.fem import ops, mixed
    for fn in (ops.solve, mixed.solve, mixed.newton_solve):
        p = inspect.signature(fn).parameters['nullspace']
        assert p.default is None
    assert ops.SolveInfo(0, 0.0, 'cg').rhs_defect is None
    assert ops.NewtonInfo(False, 'x').rhs_defect is None
    for name in ('VectorSpaceBasis', 'constant_nullspace', 'rigid_body_modes'):
        assert getattr(fem, name) is getattr(nullspace, name)


# -- the entry point ------------------------------------------------------------------
def test_flow_deflate_declared_bound_and_refusing():
    from flow_amd import _hip
    with open(os.path.join(ROOT, 'include', 'flow_hip.h')) as f:
        header = f.read()
    lib = _hip.load_library()
    assert lib.flow_abi_version() == _hip.ABI_VERSION
    assert 'int flow_deflate(' in header
    decl = header[header.index('int flow_deflate('):]
    assert decl[:decl.index(';')].count(',') == 7
    assert len(_hip.SYMBOLS['flow_deflate']) == 8
    assert _hip.SYMBOLS['flow_deflate'][3] is ctypes.c_size_t
    with open(os.path.join(ROOT, 'flow_amd', 'csrc', 'Makefile')) as f:
        assert 'nullspace_kernels.hip' in f.read()
    # nothing to do
    assert lib.flow_deflate(0, 3, None, 0, None, None, None, None) == 0
    assert lib.flow_deflate(5, 0, None, 6, None, None, None, None) == 0
    # refusals launch nothing, so host memory serves to provoke them
    before = _hip.launch_count()
    big = (ctypes.c_double * (9 * 1024 + 64))()
    base = ctypes.addressof(big)
    base += (-base) % 16
    at = lambda i: ctypes.c_void_p(base + 8 * i)   # noqa: E731
    Z, x, coef, work = at(0), at(16), at(32), at(48)
    assert lib.flow_deflate(5, 9, Z, 6, x, work, coef, None) == 2    # k > 8
    assert b'k <= 8' in lib.flow_last_error()
    assert lib.flow_deflate(5, 1, Z, 5, x, work, coef, None) == 2    # odd ldz
    assert lib.flow_deflate(5, 1, Z, 4, x, work, coef, None) == 2    # ldz < n
    assert b'ldz' in lib.flow_last_error()
    assert lib.flow_deflate(5, 1, at(1), 6, x, work, coef, None) == 2
    assert b'aligned' in lib.flow_last_error()
    assert lib.flow_deflate(5, 1, Z, 6, at(17), work, coef, None) == 2
    assert b'aligned' in lib.flow_last_error()
    for args, what in (
            ((5, 2, Z, 6, at(10), work, coef), b'x overlaps Z'),
            ((5, 1, Z, 6, Z, work, coef), b'x overlaps Z'),
            ((5, 1, Z, 6, x, at(4), coef), b'work overlaps Z'),
            ((5, 1, Z, 6, x, x, coef), b'work overlaps x'),
            ((5, 1, Z, 6, x, at(18), coef), b'work overlaps x'),
            ((5, 1, Z, 6, x, work, at(4)), b'coef overlaps Z'),
            ((5, 1, Z, 6, x, work, at(20)), b'coef overlaps x'),
            ((5, 2, Z, 6, x, work, at(48 + 2047)), b'coef overlaps work')):
        assert lib.flow_deflate(*(args + (None,))) == 2, what
        assert what in lib.flow_last_error(), (what, lib.flow_last_error())
    assert lib.flow_deflate(5, 1, None, 6, x, work, coef, None) == 2
    assert _hip.launch_count() == before
