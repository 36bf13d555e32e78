# -*- coding: utf-8 -*-
'''
fem.Projection without a GPU: the pair list against the brute force of
tests/projection_reference.py, the restatement's own identities -- every
condition tests/test_projection_gpu.py puts on the device holds for the
restatement alone, on every mesh pair named there --, the refusals that are
raised before the device is touched, and the ABI.
'''
import os

import numpy
import pytest

from flow_amd import fem
from flow_amd.fem import Projection, projection

import projection_reference as pref
import transfer_reference as tref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _space(mesh, deg, dim):
    return fem.FunctionSpace(mesh, 'CG', deg, dim=dim)


def _lin(x, y):
    return 3.0 + x - 2.0 * y


def _quad(x, y):
    return 1.0 + 2.0 * x - 3.0 * y + 0.5 * x * x + x * y - 2.0 * y * y


def _wave(x, y):
    return numpy.sin(5 * x) * numpy.cos(3 * y) + 1.5


def _wave2(x, y):
    return numpy.exp(x - y) * numpy.cos(4 * x * y) - 0.25


# -- the mesh pairs ---------------------------------------------------------------
def test_mesh_pairs_are_what_the_tests_say():
    m = pref.meshes()
    base, nested = m['base'], m['nested']
    # about a third of the cells marked
    cen = base.points[base.cell_vertices].mean(axis=1)
    marked = int((cen.sum(axis=1) < 0.9).sum())
    assert 0.25 <= marked / base.num_cells() <= 0.45
    assert nested.num_cells() > base.num_cells()
    # more than 256 target cells, no multiple of 64
    nc = m['many_to'].num_cells()
    assert nc > 256 and nc % 64 != 0


# -- the pair list ------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(pref.PAIRS))
def test_pair_list_against_brute_force(name):
    mesh_from, mesh_to, sm = pref.pair(name)
    pptr, psrc = projection.pair_list(mesh_from, mesh_to)
    nc = mesh_to.num_cells()
    assert pptr.dtype == numpy.int32 and psrc.dtype == numpy.int32
    assert pptr.shape == (nc + 1,) and pptr[0] == 0 and pptr[-1] == len(psrc)
    assert (numpy.diff(pptr) >= 0).all()
    assert psrc.min() >= 0 and psrc.max() < mesh_from.num_cells()
    listed = set()
    for t in range(nc):
        row = psrc[pptr[t]:pptr[t + 1]]
        assert (numpy.diff(row) > 0).all()       # ascending, no duplicates
        listed.update((t, int(s)) for s in row)
    # every pair that meets in positive area (above the rounding of an area
    # of cells of size ~0.1: 1e-17) is listed ...
    positive = sm.positive_pairs(1e-15)
    assert positive and positive <= listed
    # ... and the list narrows: far fewer than all pairs
    assert len(psrc) < 0.5 * nc * mesh_from.num_cells()


def test_pair_list_outside_the_source_grid():
    '''Target cells outside the source mesh's bounding box get empty rows.'''
    src = fem.UnitSquareMesh(3, 3)
    dst = fem.RectangleMesh(fem.Point(0.5, 0.5), fem.Point(2.0, 2.0), 3, 3)
    pptr, psrc = projection.pair_list(src, dst)
    sm = pref.supermesh(src, dst)
    per = numpy.diff(pptr)
    assert (per[sm.coverage == 0.0] == 0).sum() > 0
    listed = {(t, int(s)) for t in range(dst.num_cells())
              for s in psrc[pptr[t]:pptr[t + 1]]}
    assert sm.positive_pairs(1e-15) <= listed


# -- the restatement's own identities -------------------------------------------------
@pytest.mark.parametrize('name', pref.COVERED)
def test_reference_coverage_is_one(name):
    _, _, sm = pref.pair(name)
    assert numpy.abs(sm.coverage - 1.0).max() <= 1e-12


def test_reference_partial_coverage():
    '''Pair 4: partly covered cells, none uncovered, no slivers -- no cell
    has to be left out of the device's comparison.'''
    _, mesh_to, sm = pref.pair('partial')
    cov = sm.coverage
    assert (cov < projection.FULL).sum() >= 10
    assert cov.min() > 0.1
    assert not (cov < 1e-9).any()
    assert cov.max() <= 1.0 + 1e-12


@pytest.mark.parametrize('name', pref.COVERED)
@pytest.mark.parametrize('deg_to', [1, 2])
@pytest.mark.parametrize('deg_from', [1, 2])
def test_reference_load_sums_to_the_integral(name, deg_from, deg_to):
    '''sum_i b_i = int u dx (the phi_i sum to 1) and the projection keeps it.'''
    mesh_from, mesh_to, sm = pref.pair(name)
    V_from, V_to = _space(mesh_from, deg_from, 2), _space(mesh_to, deg_to, 2)
    u = pref.nodal(V_from, (_wave, _wave2))
    want = pref.integral(V_from, u)
    b = sm.load(V_from, V_to, u).reshape(2, V_to.N)
    assert numpy.abs(b.sum(axis=1) - want).max() <= 1e-13 * numpy.abs(want).max()
    w = sm.project(V_from, V_to, u)
    got = pref.integral(V_to, w)
    assert numpy.abs(got - want).max() <= 1e-11 * numpy.abs(want).max()


@pytest.mark.parametrize('name', pref.COVERED)
def test_reference_reproduces_polynomials(name):
    mesh_from, mesh_to, sm = pref.pair(name)
    for deg, f in ((1, _lin), (2, _quad)):
        V_from, V_to = _space(mesh_from, deg, 1), _space(mesh_to, deg, 1)
        w = sm.project(V_from, V_to, pref.nodal(V_from, (f,)))
        assert numpy.abs(w - pref.nodal(V_to, (f,))).max() <= 1e-10
    # a P1 field is a P2 field
    V_from, V_to = _space(mesh_from, 1, 1), _space(mesh_to, 2, 1)
    w = sm.project(V_from, V_to, pref.nodal(V_from, (_lin,)))
    assert numpy.abs(w - pref.nodal(V_to, (_lin,))).max() <= 1e-10


@pytest.mark.parametrize('deg', [1, 2])
def test_reference_same_space_is_the_identity(deg):
    mesh, _, sm = pref.pair('same')
    V = _space(mesh, deg, 2)
    u = pref.nodal(V, (_wave, _wave2))
    assert numpy.abs(sm.project(V, V, u) - u).max() <= 1e-10


def gaussian(x, y):
    '''Narrow against the coarse cells (h = 0.25), resolved by neither mesh
    well: what interpolation aliases.'''
    return numpy.exp(-((x - 0.27)**2 + (y - 0.31)**2) / (2 * 0.05**2))


@pytest.mark.parametrize('deg', [1, 2])
def test_reference_interpolation_loses_what_projection_keeps(deg):
    '''Fine -> coarse with a narrow Gaussian: the integral error of
    interpolation is at least 100 x that of the projection.'''
    mesh_from, mesh_to, sm = pref.pair('fine_to_coarse')
    V_from, V_to = _space(mesh_from, deg, 1), _space(mesh_to, deg, 1)
    u = pref.nodal(V_from, (gaussian,))
    want = pref.integral(V_from, u)[0]
    proj = abs(pref.integral(V_to, sm.project(V_from, V_to, u))[0] - want)
    interp = abs(pref.integral(V_to, tref.transfer(V_from, V_to, u))[0] - want)
    print('P%d: integral %.6e  projection error %.2e  interpolation error '
          '%.2e' % (deg, want, proj, interp))
    assert proj <= 1e-11 * abs(want)
    assert interp >= 1e-2 * abs(want)
    assert interp >= 100.0 * proj


def test_reference_scaled_load_on_partial_coverage():
    '''With the 1 / coverage scaling every target cell carries |T| times the
    source's mean over its covered part: int w dx = sum_T |T| mean_T(u), for
    u = 1 the area of the target mesh.  (Not pointwise: the weights phi_i /
    coverage over a part of T are not those of T.)'''
    mesh_from, mesh_to, sm = pref.pair('partial')
    V_from, V_to = _space(mesh_from, 1, 1), _space(mesh_to, 2, 1)
    one = numpy.ones(V_from.N)
    area = mesh_to.cell_areas().sum()
    w = sm.project(V_from, V_to, one, scale=True)
    assert abs(pref.integral(V_to, w)[0] - area) <= 1e-11 * area
    # unscaled, the partly covered cells lose mass
    assert pref.integral(V_to, sm.project(V_from, V_to, one))[0] < area - 1e-3


def test_reference_clip_by_hand():
    tri = numpy.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]])
    # itself: the triangle
    assert abs(pref.signed_area(pref.clip([tuple(p) for p in tri], tri)) - 0.5) < 1e-16
    # a shifted copy: the similar triangle of side 1/2
    moved = [tuple(p + [0.5, 0.0]) for p in tri]
    assert abs(pref.signed_area(pref.clip(moved, tri)) - 0.125) < 1e-16
    # apart: nothing
    assert len(pref.clip([tuple(p + [2.0, 2.0]) for p in tri], tri)) < 3
    # a hexagon: two triangles pointing opposite ways
    up = numpy.array([[0.0, 0.0], [3.0, 0.0], [1.5, 3.0]])
    down = [(0.0, 2.0), (1.5, -1.0), (3.0, 2.0)]
    assert len(pref.clip(down, up)) == 6


# -- refusals ---------------------------------------------------------------------
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
            Projection(a, b)
    for a, b in ((W, P2), (P1, W)):
        with pytest.raises(ValueError, match='component'):
            Projection(a, b)
    # a Projection that was set up (here: without its device parts) refuses
    # operands of other spaces before anything is launched
    P = Projection.__new__(Projection)
    P.V_from, P.V_to = P2, P1
    for bad in (fem.Function(P1), fem.Function(W),
                fem.Function(_space(other, 2, 1)), 3.0, fem.Constant(1.0)):
        with pytest.raises(ValueError, match='u_from'):
            P.apply(bad)
        with pytest.raises(ValueError, match='u_from'):
            P.load(bad)
    u = fem.Function(P2)
    for bad in (fem.Function(P2), fem.Function(_space(other, 1, 1)), 3.0):
        with pytest.raises(ValueError, match='out'):
            P.apply(u, out=bad)
    with pytest.raises(ValueError, match='not a Function'):
        fem.project_onto(fem.Constant(1.0), P1)
    from flow_amd import parallel
    monkeypatch.setattr(parallel, 'active', lambda: True)
    for call in (lambda: Projection(P2, P1), lambda: P.apply(u),
                 lambda: P.load(u), lambda: fem.project_onto(u, P1)):
        with pytest.raises(NotImplementedError, match='on strips'):
            call()


def test_exports():
    assert fem.Projection is projection.Projection
    assert fem.project_onto is projection.project_onto


def test_symbol_declared_and_bound():
    from flow_amd import _hip
    with open(os.path.join(ROOT, 'include', 'flow_hip.h')) as f:
        header = f.read()
    lib = _hip.load_library()
    assert lib.flow_abi_version() == 30 == _hip.ABI_VERSION
    name, nargs = 'flow_project_load', 14
    assert 'int %s(' % name in header
    assert len(_hip.SYMBOLS[name]) == nargs
    decl = header[header.index('int %s(' % name):]
    assert decl[:decl.index(';')].count(',') == nargs - 1
    assert getattr(lib, name) is not None
