# -*- coding: utf-8 -*-
'''
Gradient recovery without a GPU (flow_amd/fem/recovery.py): the numpy
restatement (tests/recovery_reference.py) on fields it must reproduce exactly,
the space's contribution map against the patches the restatement finds, the
refusals (all raised before the device is touched), the exports, the symbols,
and the superconvergence inequalities the GPU test asserts, checked here for
the restatement.

Exactness.  The P_k interpolant of a global polynomial of degree k is that
polynomial in every cell, so every cell of a patch gives the exact gradient
at the node and any weighted mean of them is exact: interior and boundary
nodes alike, to rounding (1e-12 against gradients of size 1 to 10).
'''
import os

import numpy
import pytest

from flow_amd import fem

import recovery_reference as rref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _space(name, deg, dim):
    return fem.FunctionSpace(rref.mesh(name), 'CG', deg, dim=dim)


def _boundary_nodes(V):
    '''bool (N,): nodes on boundary facets (vertices and edge mid points).'''
    mesh = V.mesh()
    on = numpy.zeros(V.N, dtype=bool)
    on[V.layout.vertex_dofs[numpy.unique(mesh.edges[mesh.bfacets])]] = True
    if V.degree == 2:
        on[V.layout.edge_dofs[mesh.bfacets]] = True
    return on


# -- the restatement on polynomials ------------------------------------------------
@pytest.mark.parametrize('dim', [1, 2])
@pytest.mark.parametrize('deg', [1, 2])
@pytest.mark.parametrize('name', rref.MESHES)
def test_reference_is_exact_for_polynomials_of_the_degree(name, deg, dim):
    V = _space(name, deg, dim)
    funcs, grads, gmax = rref.EXACT[(deg, dim)]
    u = rref.field(V, funcs)
    G = rref.gradient(u)
    assert G.shape == (dim, 2, V.N)
    xy = V.layout.dof_coords
    want = numpy.array([numpy.broadcast_arrays(*g(xy[:, 0], xy[:, 1]))
                        for g in grads])
    err = numpy.abs(G - want).max(axis=(0, 1))
    on = _boundary_nodes(V)
    assert on.any() and (~on).any()
    print('%s P%d x%d: interior %.2e boundary %.2e'
          % (name, deg, dim, err[~on].max(), err[on].max()))
    assert err[~on].max() <= 1e-12 and err[on].max() <= 1e-12
    area = numpy.abs(V.mesh().cell_areas()).sum()
    eta2 = rref.indicator(u, G)
    assert eta2.shape == (V.mesh().num_cells(),)
    assert eta2.max() <= 1e-22 * gmax**2 * area


def test_reference_sees_a_field_that_is_not_in_the_space():
    '''... and is no constant zero: a quadratic on P1 leaves eta2 > 0 in
    every cell, and the vector indicator is the sum of its components'.'''
    mesh = rref.mesh('fitted hole')
    V = fem.FunctionSpace(mesh, 'CG', 1)
    W = fem.VectorFunctionSpace(mesh, 'CG', 1)
    a, b = rref.field(V, [rref.quadratic]), rref.field(V, [rref.quadratic1])
    w = rref.field(W, [rref.quadratic, rref.quadratic1])
    ea, eb, ew = rref.indicator(a), rref.indicator(b), rref.indicator(w)
    assert ea.min() > 0.0 and eb.min() > 0.0
    assert numpy.abs(ew - (ea + eb)).max() <= 1e-14 * ew.max()
    Gw = rref.gradient(w)
    assert numpy.array_equal(Gw[0], rref.gradient(a)[0])
    assert numpy.array_equal(Gw[1], rref.gradient(b)[0])


# -- the contribution map ------------------------------------------------------------
@pytest.mark.parametrize('deg', [1, 2])
@pytest.mark.parametrize('name', rref.MESHES)
def test_contribution_map_lists_the_patches(name, deg):
    V = _space(name, deg, 1)
    nc = V.mesh().num_cells()
    vptr, vsrc = V.layout.vmap('vptr'), V.layout.vmap('vsrc')
    assert vptr.shape == (V.N + 1,) and vptr[0] == 0
    assert vptr[-1] == len(vsrc) == V.layout.nloc * nc
    assert (numpy.diff(vptr) >= 1).all()
    want = rref.patches(V)
    sizes = set()
    for n in range(V.N):
        s = vsrc[vptr[n]:vptr[n + 1]]
        got = sorted(zip((s // nc).tolist(), (s % nc).tolist()))
        assert got == sorted(want[n]), n
        sizes.add(len(got))
    print('%s P%d: patches of %s cells' % (name, deg, sorted(sizes)))
    if name == 'square 2':
        # one interior vertex (six cells); every other vertex patch one-sided
        on = _boundary_nodes(V)
        assert (~on[V.layout.vertex_dofs]).sum() == 1


# -- refusals, exports, symbols --------------------------------------------------------
def test_refusals(monkeypatch):
    mesh = fem.UnitSquareMesh(4, 4)
    other = fem.UnitSquareMesh(4, 4)
    P1, P2 = fem.FunctionSpace(mesh, 'CG', 1), fem.FunctionSpace(mesh, 'CG', 2)
    W = fem.VectorFunctionSpace(mesh, 'CG', 2)
    W1 = fem.VectorFunctionSpace(mesh, 'CG', 1)
    mixed = fem.FunctionSpace(
        mesh, fem.VectorElement('CG', 'triangle', 2)
        * fem.FiniteElement('CG', 'triangle', 1))
    for V in (mixed, W.sub(0), W.sub(1)):
        with pytest.raises(NotImplementedError):
            fem.GradientRecovery(V)

    class Cubic(object):
        layout, component, degree, dim = P2.layout, None, 3, 1

    class Triple(object):
        layout, component, degree, dim = P2.layout, None, 2, 3

    with pytest.raises(ValueError, match='P3'):
        fem.GradientRecovery(Cubic())
    with pytest.raises(ValueError, match='3 components'):
        fem.GradientRecovery(Triple())
    R = fem.GradientRecovery(P2)
    assert R.G.same_as(W)
    for bad in (fem.Function(P1), fem.Function(W),
                fem.Function(fem.FunctionSpace(other, 'CG', 2)), 3.0,
                fem.Constant(1.0)):
        for call in (R.apply, R.indicator, R.estimate):
            with pytest.raises(ValueError, match='u:'):
                call(bad)
    u = fem.Function(P2)
    for bad in (fem.Function(P2), fem.Function(W1),
                fem.Function(fem.VectorFunctionSpace(other, 'CG', 2)),
                (fem.Function(W), fem.Function(W)), 3.0):
        with pytest.raises(ValueError, match='out:'):
            R.apply(u, out=bad)
    RW = fem.GradientRecovery(W)
    w, g = fem.Function(W), fem.Function(W)
    for bad in (g, (g,), (g, fem.Function(W1)), (g, g), [g, fem.Function(P2)]):
        with pytest.raises(ValueError, match='out:'):
            RW.apply(w, out=bad)
    from flow_amd import parallel
    monkeypatch.setattr(parallel, 'active', lambda: True)
    for call in (lambda: fem.GradientRecovery(P2), lambda: R.apply(u),
                 lambda: R.indicator(u), lambda: R.estimate(u),
                 lambda: fem.recover_gradient(fem.Function(P1)),
                 lambda: fem.zz_indicator(fem.Function(P1))):
        with pytest.raises(NotImplementedError, match='on strips'):
            call()


def test_exports():
    from flow_amd.fem import recovery
    for name in ('GradientRecovery', 'recover_gradient', 'zz_indicator'):
        assert getattr(fem, name) is getattr(recovery, name)


def test_symbols_declared_and_bound():
    from flow_amd import _hip
    with open(os.path.join(ROOT, 'include', 'flow_hip.h')) as f:
        header = f.read()
    lib = _hip.load_library()
    assert lib.flow_abi_version() == 30 == _hip.ABI_VERSION
    for name, nargs in (('flow_recover_gradient', 6), ('flow_zz_indicator', 9)):
        assert 'int %s(' % name in header
        assert len(_hip.SYMBOLS[name]) == nargs
        decl = header[header.index('int %s(' % name):]
        assert decl[:decl.index(';')].count(',') == nargs - 1
        assert getattr(lib, name) is not None


# -- superconvergence of the restatement -----------------------------------------------
def test_reference_recovered_gradient_is_superconvergent():
    '''What tests/test_recovery_gpu.py asserts of the device holds for the
    restatement: on UnitSquareMesh(8, 8) and (16, 16), P1 interpolant of
    sin(pi x) sin(pi y), the recovered gradient is nearer to the exact one
    than the cell gradient is, and gains more from the refinement.'''
    rows = []
    for n in (8, 16):
        V = fem.FunctionSpace(fem.UnitSquareMesh(n, n), 'CG', 1)
        u = rref.field(V, [rref.bubble])
        rows.append(rref.gradient_errors(u, rref.bubble_grad))
    print('recovered %.4e -> %.4e (x %.2f), raw %.4e -> %.4e (x %.2f)'
          % (rows[0][0], rows[1][0], rows[0][0] / rows[1][0],
             rows[0][1], rows[1][1], rows[0][1] / rows[1][1]))
    for rec, raw in rows:
        assert rec < raw
    assert rows[0][0] / rows[1][0] > rows[0][1] / rows[1][1]
