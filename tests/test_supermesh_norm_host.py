# -*- coding: utf-8 -*-
'''
fem.Supermesh without a GPU: the identities of the numpy restatement of
tests/supermesh_norm_reference.py alone (what tests/test_supermesh_norm_gpu.py
compares the device with), the conditions on the partly covered mesh pair,
the refusals raised before the device is touched, and the ABI.
'''
import os

import numpy
import pytest

from flow_amd import fem
from flow_amd.fem import Supermesh, projection, supermesh

import supermesh_norm_reference as sref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEGREES = [(1, 1), (1, 2), (2, 1), (2, 2)]


def _space(mesh, deg, dim):
    return fem.FunctionSpace(mesh, 'CG', deg, dim=dim)


def _x(x, y):
    return x + 0.0 * y


def _y(x, y):
    return y + 0.0 * x


def _quad(x, y):
    return 1.0 + 2.0 * x - 3.0 * y + 0.5 * x * x + x * y - 2.0 * y * y


def _quad2(x, y):
    return -0.5 + x - y + 3.0 * x * x - 2.0 * x * y + y * y


def _wave(x, y):
    return numpy.sin(5 * x) * numpy.cos(3 * y) + 1.5


def _wave2(x, y):
    return numpy.exp(x - y) * numpy.cos(4 * x * y) - 0.25


# -- the restatement alone ------------------------------------------------------------
@pytest.mark.parametrize('deg_a,deg_b', DEGREES)
@pytest.mark.parametrize('name', sref.COVERED)
def test_reference_x_against_y(name, deg_a, deg_b):
    '''On the unit square int (x - y)^2 = 1/6 and int |(1, -1)|^2 = 2; int x y
    = 1/4 and grad x . grad y = 0.'''
    mesh_a, mesh_b, _ = sref.pair(name)
    V_a, V_b = _space(mesh_a, deg_a, 1), _space(mesh_b, deg_b, 1)
    r = sref.norms(name, V_a, V_b, sref.pref.nodal(V_a, (_x,)),
                   sref.pref.nodal(V_b, (_y,)))
    assert abs(r['l2'].sum() - 1.0 / 6.0) <= 1e-13
    assert abs(r['h10'].sum() - 2.0) <= 1e-13
    assert abs(r['uw'].sum() - 0.25) <= 1e-13
    assert abs(r['gugw'].sum()) <= 1e-13
    assert abs(r['area'] - 1.0) <= 1e-13
    assert (r['l2'] >= 0.0).all() and (r['h10'] >= 0.0).all()


@pytest.mark.parametrize('name', sref.COVERED)
def test_reference_quadratic_against_its_interpolant(name):
    '''A quadratic lies in P2 of either mesh: the error between its two
    nodal interpolants is 0, for both components of a vector field.'''
    mesh_a, mesh_b, _ = sref.pair(name)
    V_a, V_b = _space(mesh_a, 2, 2), _space(mesh_b, 2, 2)
    r = sref.norms(name, V_a, V_b, sref.pref.nodal(V_a, (_quad, _quad2)),
                   sref.pref.nodal(V_b, (_quad, _quad2)))
    assert r['l2'].sum() <= 1e-13
    assert r['h10'].sum() <= 1e-13


@pytest.mark.parametrize('name,back', [('coarse_to_fine', 'fine_to_coarse'),
                                       ('same', 'same')])
def test_reference_does_not_depend_on_the_roles(name, back):
    '''The integrals over the overlap with the two spaces in either role:
    other target cells, other clips, the same sums.'''
    mesh_a, mesh_b, _ = sref.pair(name)
    assert sref.pair(back)[:2] == (mesh_b, mesh_a)
    V_a, V_b = _space(mesh_a, 2, 2), _space(mesh_b, 1, 2)
    u = sref.pref.nodal(V_a, (_wave, _wave2))
    w = sref.pref.nodal(V_b, (_wave2, _wave))
    r = sref.norms(name, V_a, V_b, u, w)
    q = sref.norms(back, V_b, V_a, w, u)
    for key in ('uw', 'gugw', 'l2', 'h10'):
        assert abs(q[key].sum() - r[key].sum()) <= 1e-12 * abs(r[key].sum())
    # |u - w|^2 = |u|^2 - 2 u w + |w|^2 on one mesh
    if name == 'same':
        uu = sref.norms(name, V_a, V_a, u, u)
        ww = sref.norms(name, V_b, V_b, w, w)
        assert uu['l2'].sum() <= 1e-13 * uu['uw'].sum()
        for sq, pr in (('l2', 'uw'), ('h10', 'gugw')):
            want = uu[pr].sum() - 2.0 * r[pr].sum() + ww[pr].sum()
            assert abs(r[sq].sum() - want) <= 1e-12 * uu[pr].sum()


def test_reference_partial_pair():
    '''rectangle_with_hole 9 x 9 -> 12 x 10 'left': partly covered cells,
    the least covered to about 0.40, and none uncovered -- no cell is left
    out of the device's comparison.'''
    mesh_a, mesh_b, sm = sref.pair('partial')
    V_a, V_b = _space(mesh_a, 2, 1), _space(mesh_b, 1, 1)
    r = sref.norms('partial', V_a, V_b, sref.pref.nodal(V_a, (_wave,)),
                   sref.pref.nodal(V_b, (_wave2,)))
    cov = r['coverage']
    assert (cov < projection.FULL).sum() >= 10
    assert abs(cov.min() - 0.40) < 0.01
    assert not (cov < 1e-9).any()
    assert cov.max() <= 1.0 + 1e-12
    total = mesh_b.cell_areas().sum()
    assert abs(r['area'] - (cov * mesh_b.cell_areas()).sum()) <= 1e-13
    assert r['area'] < total - 1e-3
    # the partly covered cells carry their share of the integrals
    assert (r['l2'][cov < projection.FULL] > 0.0).all()


def test_reference_gradients_by_hand():
    v = numpy.array([[[0.0, 0.0], [2.0, 0.0], [0.0, 4.0]]])
    g = sref.bary_gradients(v)[0]
    assert numpy.allclose(g, [[-0.5, -0.25], [0.5, 0.0], [0.0, 0.25]], atol=1e-15)
    # the derivatives of the bases against differences of the bases
    rng = numpy.random.RandomState(3)
    L = rng.rand(5, 3)
    h = 1e-6
    for deg in (1, 2):
        d = sref.dbasis(deg, L)
        for k in range(3):
            e = numpy.zeros(3)
            e[k] = h
            fd = (sref.pref.basis(deg, L + e) - sref.pref.basis(deg, L - e)) / (2 * h)
            assert numpy.abs(d[..., k] - fd).max() <= 1e-9


def test_device_order_sum_by_hand():
    '''Integers sum exactly in any order; a length that needs two blocks
    and one that needs every lane twice (more than 1024 blocks' worth).'''
    for n in (1, 8, 255, 264, 1000, 256 * 1024 + 77):
        x = numpy.arange(1, n + 1, dtype=numpy.float64)
        assert sref.sum_in_device_order(x) == n * (n + 1) / 2.0
    x = numpy.random.RandomState(5).rand(264)
    assert abs(sref.sum_in_device_order(x) - x.sum()) <= 1e-13 * x.sum()
    # the order is a fixed one, not numpy's: the halves of a wave are paired
    y = numpy.zeros(64)
    y[0], y[32], y[1] = 1.0, 2.0**-53, 2.0**-53
    assert sref.sum_in_device_order(y) == 1.0          # (1 + e) + ... rounds twice
    assert y[[1, 32, 0]].sum() > 1.0


# -- refusals -----------------------------------------------------------------------
def test_refusals(monkeypatch):
    mesh = fem.UnitSquareMesh(4, 4)
    other = fem.UnitSquareMesh(4, 4)
    P1, P2 = _space(mesh, 1, 1), _space(mesh, 2, 1)
    W = _space(mesh, 2, 2)
    mixed = fem.FunctionSpace(
        mesh, fem.VectorElement('CG', 'triangle', 2)
        * fem.FiniteElement('CG', 'triangle', 1))
    for a, b in ((W.sub(0), P2), (P2, W.sub(1)), (mixed, P2), (W, mixed)):
        with pytest.raises(NotImplementedError):
            Supermesh(a, b)
    for a, b in ((W, P2), (P1, W)):
        with pytest.raises(ValueError, match='component'):
            Supermesh(a, b)
    # a Supermesh that was set up (here: without its device parts) refuses a
    # bad norm_type and operands of other spaces before anything is launched
    S = Supermesh.__new__(Supermesh)
    S.V_a, S.V_b, S.nc = P2, P1, mesh.num_cells()
    u, w = fem.Function(P2), fem.Function(P1)
    for call in (S.cell_errors, S.errornorm, S.inner):
        for bad in ('l2', 'H2', 'linf', None, 2):
            with pytest.raises(ValueError, match='norm_type'):
                call(u, w, bad)
        for bad in (fem.Function(P1), fem.Function(W),
                    fem.Function(_space(other, 2, 1)), 3.0, fem.Constant(1.0)):
            with pytest.raises(ValueError, match='u: not a Function'):
                call(bad, w)
        for bad in (fem.Function(P2), fem.Function(_space(other, 1, 1)), 3.0):
            with pytest.raises(ValueError, match='w: not a Function'):
                call(u, bad)
    with pytest.raises(ValueError, match='out'):
        S.cell_errors(u, w, out=numpy.zeros(3))
    with pytest.raises(ValueError, match='norm_type'):
        fem.mesh_errornorm(u, w, 'max')
    with pytest.raises(ValueError, match='not a Function'):
        fem.mesh_errornorm(fem.Constant(1.0), w)
    from flow_amd import parallel
    monkeypatch.setattr(parallel, 'active', lambda: True)
    for call in (lambda: Supermesh(P2, P1), lambda: S.cell_errors(u, w),
                 lambda: S.errornorm(u, w, 'H1'), lambda: S.inner(u, w),
                 lambda: fem.mesh_errornorm(u, w)):
        with pytest.raises(NotImplementedError, match='on strips'):
            call()


def test_exports():
    assert fem.Supermesh is supermesh.Supermesh
    assert fem.mesh_errornorm is supermesh.mesh_errornorm
    assert supermesh.NORMS == ('L2', 'H10', 'H1')


def test_symbol_declared_and_bound():
    from flow_amd import _hip
    with open(os.path.join(ROOT, 'include', 'flow_hip.h')) as f:
        header = f.read()
    lib = _hip.load_library()
    assert lib.flow_abi_version() == 30 == _hip.ABI_VERSION
    name, nargs = 'flow_supermesh_norms', 15
    assert 'int %s(' % name in header
    assert len(_hip.SYMBOLS[name]) == nargs
    decl = header[header.index('int %s(' % name):]
    assert decl[:decl.index(';')].count(',') == nargs - 1
    assert getattr(lib, name) is not None
