# -*- coding: utf-8 -*-
'''
fem.BoundaryProfile, the host side (flow_amd/fem/profile.py): curve
construction against the numpy restatement of tests/profile_reference.py,
`crossings` on hand-made rows, the refusals, and the two symbols of the C
ABI.  No GPU.
'''
import ctypes
import os

import numpy
import pytest

from flow_amd import fem, parallel
from flow_amd.fem import (
    FacetNormal, MeshFunction, TestFunction, TrialFunction, dot, grad,
    )

import profile_reference as pref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOLE = (0.0, 1.0, 0.0, 0.5, (0.4, 0.25), 0.12, 18, 9)


def _turning(P, c):
    '''Signed area enclosed by the facets of closed curve c (shoelace over
    the samples' facets: > 0 counter-clockwise).'''
    pts = P.x[:, P.curve_points(c)]
    x, y = pts
    return 0.5 * float(numpy.sum(x * numpy.roll(y, -1) - numpy.roll(x, -1) * y))


def _same_as_reference(P, mesh, pos, degree, start=None):
    R = pref.Reference(mesh, pos, degree, start)
    assert P.num_curves == len(R.curves)
    assert numpy.array_equal(P.curve_facets, R.offsets)
    assert numpy.array_equal(P.closed, R.closed)
    assert numpy.array_equal(P.facet_index, R.order)
    assert numpy.array_equal(P.facet_cell, mesh.bfacet_cell[R.order])
    assert numpy.array_equal(P.facet_local, mesh.bfacet_local[R.order])
    assert numpy.abs(P.facet_length - R.length).max() < 1e-15
    assert numpy.abs(P.x - R.x).max() < 1e-15
    assert numpy.abs(P.s - R.s).max() < 1e-14
    assert numpy.abs(P.weights - R.weights).max() < 1e-16
    assert numpy.abs(numpy.repeat(P.normal, P.m, axis=1) - R.normal).max() < 1e-15
    return R


def test_unit_square():
    mesh = fem.UnitSquareMesh(2, 2)
    P = fem.BoundaryProfile(mesh)
    assert P.num_curves == 1 and P.closed.tolist() == [True]
    assert P.curve_facets.tolist() == [0, 8] and P.nfacets == 8
    assert P.m == 2 and P.npoints == 16 and P.x.shape == (2, 16)
    # from (0, 0) along the lower side: counter-clockwise
    assert P.x[1, 0] == 0.0 and 0.0 < P.x[0, 0] < P.x[0, 1] < 0.5
    assert numpy.all(numpy.diff(P.s) > 0.0)
    assert _turning(P, 0) > 0.0
    assert abs(P.facet_length.sum() - 4.0) < 1e-15
    # s ends one Gauss offset short of the perimeter, at the start vertex
    t = fem.reference.line_rule(2)[0]
    assert abs(P.s[-1] - (4.0 - 0.5 * (1.0 - t[-1]))) < 1e-14
    assert abs(P.x[0, -1]) < 1e-15 and P.x[1, -1] < 0.5
    assert P.normal[:, 0].tolist() == [0.0, -1.0]
    _same_as_reference(P, mesh, range(len(mesh.bfacets)), 2)
    ang = P.angle((0.5, 0.5))
    assert numpy.allclose(ang, numpy.arctan2(P.x[1] - 0.5, P.x[0] - 0.5))


def test_rectangle_with_hole():
    mesh = fem.rectangle_with_hole(*HOLE)
    P = fem.BoundaryProfile(mesh, degree=6)
    assert P.num_curves == 2 and P.closed.all() and P.m == 4
    # the outer boundary first (it starts at (0, 0)), counter-clockwise; the
    # hole clockwise
    assert _turning(P, 0) > 0.0 > _turning(P, 1)
    lo, mid, hi = P.curve_facets
    assert abs(P.facet_length[lo:mid].sum() - 3.0) < 1e-14
    # the staircase: axis-parallel edges of the grid and cell diagonals
    ev = mesh.edges[mesh.bfacets[P.facet_index[mid:hi]]]
    d = mesh.points[ev[:, 1]] - mesh.points[ev[:, 0]]
    assert abs(P.facet_length[mid:hi].sum()
               - numpy.hypot(d[:, 0], d[:, 1]).sum()) < 1e-14
    inner = numpy.hypot(P.x[0] - 0.4, P.x[1] - 0.25) < 0.2
    assert inner[P.curve_points(1)].all() and not inner[P.curve_points(0)].any()
    # each curve starts at its lexicographically smallest vertex
    for c in range(2):
        v = mesh.edges[mesh.bfacets[P.facet_index[P.curve_facets[c]:
                                                  P.curve_facets[c + 1]]]]
        xy = mesh.points[numpy.unique(v)]
        first = xy[numpy.lexsort((xy[:, 1], xy[:, 0]))[0]]
        k = P.curve_facets[c]
        x0 = P.x[:, k * P.m] - (P.x[:, k * P.m + 1] - P.x[:, k * P.m]) \
            * P.s[k * P.m] / (P.s[k * P.m + 1] - P.s[k * P.m])
        assert numpy.abs(x0 - first).max() < 1e-14
    _same_as_reference(P, mesh, range(len(mesh.bfacets)), 6)


class _Left(fem.SubDomain):
    def inside(self, x, on_boundary):
        return on_boundary & (x[0] < 1e-12)


def test_marked_left_edge_is_open_and_runs_downward():
    mesh = fem.UnitSquareMesh(3, 2)
    markers = MeshFunction('size_t', mesh, 1, 0)
    _Left().mark(markers, 7)
    for where in (_Left(), (markers, 7)):
        P = fem.BoundaryProfile(mesh, where, degree=4)
        assert P.num_curves == 1 and P.closed.tolist() == [False]
        assert P.nfacets == 2 and P.m == 3
        assert numpy.all(P.x[0] == 0.0) and numpy.all(numpy.diff(P.x[1]) < 0.0)
        assert abs(P.s[-1] + (1.0 - P.x[1, 0]) - 1.0) < 1e-14
        assert numpy.array_equal(P.normal, [[-1.0, -1.0], [0.0, 0.0]])
        pos = numpy.nonzero(markers.array()[mesh.bfacets] == 7)[0]
        _same_as_reference(P, mesh, pos, 4)
    with pytest.raises(ValueError, match='another mesh'):
        fem.BoundaryProfile(fem.UnitSquareMesh(3, 2), (markers, 7))
    with pytest.raises(ValueError, match='where'):
        fem.BoundaryProfile(mesh, numpy.arange(3))


def test_start_rotates_a_closed_curve():
    mesh = fem.rectangle_with_hole(*HOLE)
    P0 = fem.BoundaryProfile(mesh)
    P1 = fem.BoundaryProfile(mesh, start=(1.0, 0.5))
    assert P1.num_curves == 2
    # the hole's first vertex now sorts before (1, 0.5): it comes first
    a0, b0 = P0.facet_index[:P0.curve_facets[1]], P0.facet_index[P0.curve_facets[1]:]
    b1, a1 = P1.facet_index[:P1.curve_facets[1]], P1.facet_index[P1.curve_facets[1]:]
    assert numpy.array_equal(b0, b1)
    k = int(numpy.nonzero(a0 == a1[0])[0][0])
    assert k > 0 and numpy.array_equal(numpy.roll(a0, -k), a1)
    first = P1.curve_facets[1] * P1.m
    # ... and the outer curve leaves (1, 0.5) along the upper side
    assert P1.x[1, first] == 0.5 and 0.9 < P1.x[0, first] < 1.0
    assert P1.s[first] < P1.facet_length[P1.curve_facets[1]]
    _same_as_reference(P1, mesh, range(len(mesh.bfacets)), 2, (1.0, 0.5))
    # a point next to the hole rotates the hole
    P2 = fem.BoundaryProfile(mesh, start=(0.52, 0.25))
    k = int(numpy.nonzero(b0 == P2.facet_index[P2.curve_facets[1]])[0][0])
    assert numpy.array_equal(numpy.roll(b0, -k),
                             P2.facet_index[P2.curve_facets[1]:])
    assert numpy.array_equal(a0, P2.facet_index[:P2.curve_facets[1]])
    _same_as_reference(P2, mesh, range(len(mesh.bfacets)), 2, (0.52, 0.25))


def test_bow_tie_vertex_is_refused():
    # two triangles that touch in one vertex only
    pts = numpy.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0], [-1.0, 0.0],
                       [0.0, -1.0]])
    mesh = fem.Mesh(pts, numpy.array([[0, 1, 2], [0, 3, 4]]))
    with pytest.raises(ValueError, match='shared by 4 selected facets'):
        fem.BoundaryProfile(mesh)


class _Nowhere(fem.SubDomain):
    def inside(self, x, on_boundary):
        return on_boundary & (x[0] < -1.0)


def test_empty_selection():
    mesh = fem.UnitSquareMesh(2, 2)
    P = fem.BoundaryProfile(mesh, _Nowhere())
    assert P.num_curves == 0 and P.nfacets == 0 and P.npoints == 0
    assert P.curve_facets.tolist() == [0] and P.closed.shape == (0,)
    assert P.x.shape == (2, 0) and P.s.shape == (0,) and P.weights.shape == (0,)
    assert P.angle((0.0, 0.0)).shape == (0,)
    assert P.crossings(numpy.zeros(0)) == []
    V = fem.FunctionSpace(mesh, 'CG', 1)
    u = fem.Function(V)
    # nothing is launched: no library, no GPU is asked for
    for call in (P.evaluate, P.integrate, P.cumulative):
        assert tuple(call(u).shape) == (1, 0)
        assert tuple(call(grad(u)).shape) == (2, 0)
    assert tuple(P.total(u).shape) == (1, 0)


def _row_profile():
    '''A closed curve of 4 facets with 2 samples each, and an open one.'''
    mesh = fem.UnitSquareMesh(1, 1)
    return fem.BoundaryProfile(mesh, degree=2), \
        fem.BoundaryProfile(mesh, _Left(), degree=2)


def test_crossings():
    P, Q = _row_profile()
    assert P.npoints == 8 and P.closed[0] and Q.npoints == 2 and not Q.closed[0]
    s = P.s
    # no crossing
    assert P.crossings(numpy.ones(8))[0].size == 0
    assert P.crossings(numpy.arange(8.0), level=-1.0)[0].size == 0
    # one change inside, one across the wrap-around
    span = s[0] + 4.0 - s[7]
    v = numpy.array([3.0, 1.0, 1.0, -1.0, -1.0, -1.0, -1.0, -1.0])
    got, = P.crossings(v)
    assert got.shape == (2,)
    assert abs(got[0] - 0.5 * (s[2] + s[3])) < 1e-15
    assert abs(got[1] - (s[7] + 0.25 * span)) < 1e-14 and s[7] < got[1] < 4.0
    # a wrap-around crossing past the start vertex comes back as a small s
    v = numpy.array([1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, -3.0])
    got, = P.crossings(v)
    assert got.shape == (2,)
    assert abs(got[0] - (s[7] + 0.75 * span - 4.0)) < 1e-14 and 0.0 <= got[0] < s[0]
    assert abs(got[1] - (s[6] + 0.25 * (s[7] - s[6]))) < 1e-14
    # the level; an exact zero sample counts once, at its own arclength
    v = numpy.array([2.0, 1.0, 0.5, 1.0, 2.0, 2.0, 2.0, 2.0])
    assert P.crossings(v)[0].size == 0
    got, = P.crossings(v, level=0.5)
    assert got.tolist() == [s[2]]
    got, = P.crossings(numpy.array([1.0, 0.0, -1.0, -1.0, -1.0, -1.0, -1.0, 0.0]))
    assert got.tolist() == [s[1], s[7]]
    # an open curve has no wrap-around pair; (1, n) rows are taken
    assert Q.crossings(numpy.array([[1.0, -1.0]]))[0].tolist() \
        == [0.5 * (Q.s[0] + Q.s[1])]
    assert Q.crossings(numpy.array([-1.0, -1.0]))[0].size == 0
    with pytest.raises(ValueError, match='samples'):
        P.crossings(numpy.zeros(7))


def test_refusals(monkeypatch):
    from flow_amd import _hip
    mesh = fem.UnitSquareMesh(2, 2)
    V = fem.FunctionSpace(mesh, 'CG', 2)
    u = fem.Function(V)
    P = fem.BoundaryProfile(mesh)
    n = FacetNormal(mesh)
    for bad in (TestFunction(V), u * TrialFunction(V),
                dot(grad(TestFunction(V)), n)):
        for call in (P.evaluate, P.integrate, P.cumulative, P.total):
            with pytest.raises(ValueError, match='test or trial function'):
                call(bad)
    other = fem.Function(fem.FunctionSpace(fem.UnitSquareMesh(2, 2), 'CG', 1))
    with pytest.raises(ValueError, match='different meshes'):
        P.evaluate(other)
    # 3 m rows of the facet rule: m = degree // 2 + 1
    limit = _hip.FORM_MAX_POINTS // 3
    assert fem.BoundaryProfile(mesh, degree=2 * (limit - 1)).m == limit
    with pytest.raises(ValueError, match='limit'):
        fem.BoundaryProfile(mesh, degree=2 * limit)
    with pytest.raises(ValueError, match='start'):
        fem.BoundaryProfile(mesh, start=(1.0, 2.0, 3.0))
    monkeypatch.setattr(parallel, 'active', lambda: True)
    with pytest.raises(NotImplementedError, match='on strips'):
        fem.BoundaryProfile(mesh)
    for call in (P.evaluate, P.integrate, P.cumulative, P.total):
        with pytest.raises(NotImplementedError, match='on strips'):
            call(u)


def test_builders_are_plain_expressions():
    from flow_amd.fem import forms
    mesh = fem.UnitSquareMesh(2, 2)
    W = fem.VectorFunctionSpace(mesh, 'CG', 2)
    Q = fem.FunctionSpace(mesh, 'CG', 1)
    u, p = fem.Function(W), fem.Function(Q)
    mu = fem.Constant(0.3)
    assert fem.traction(u, p, mu).shape == (2,)
    assert fem.wall_shear(u, mu).shape == ()
    assert fem.wall_shear(u, 0.3).shape == ()
    assert fem.pressure_coefficient(p, 1.0, 2.0, fem.Constant(3.0)).shape == ()
    assert fem.normal_flux(p, 1.0 + p * p).shape == ()
    for e in (fem.traction(u, p, mu), fem.wall_shear(u, mu),
              fem.normal_flux(p, mu)):
        assert all(forms.has_normal(t) for t in e.scalar_trees())
        forms.compile_trees(e.scalar_trees()[:2], facet=True)


def test_symbols_declared_and_bound():
    from flow_amd import _hip
    with open(os.path.join(ROOT, 'include', 'flow_hip.h')) as f:
        header = f.read()
    lib = _hip.load_library()
    assert lib.flow_abi_version() == _hip.ABI_VERSION
    for name, nargs in (('flow_form_facet_values', 10),
                        ('flow_profile_cumsum', 7)):
        assert 'int %s(' % name in header
        assert len(_hip.SYMBOLS[name]) == nargs
        decl = header[header.index('int %s(' % name):]
        assert decl[:decl.index(';')].count(',') == nargs - 1
        assert getattr(lib, name) is not None
    assert '#define FLOW_PROFILE_CURVES_PER_LAUNCH %d' \
        % _hip.PROFILE_CURVES_PER_LAUNCH in header
    # argument checks that need no device: nothing to do, and bad arguments
    cum = lib.flow_profile_cumsum
    ints = lambda *v: (ctypes.c_int * len(v))(*v)
    fake = ctypes.c_void_p(4096)                # never dereferenced below
    assert cum(0, ints(0), 3, 0, None, None, None) == 0
    assert cum(2, ints(0, 0, 0), 1, 0, None, None, None) == 0
    assert cum(1, ints(0, 5), 0, 5, None, None, None) == 0
    assert cum(1, None, 1, 5, fake, fake, None) == 2
    assert cum(-1, ints(0), 1, 0, fake, fake, None) == 2
    assert cum(1, ints(0, 5), -1, 5, fake, fake, None) == 2
    assert cum(2, ints(0, 4, 3), 1, 3, fake, fake, None) == 2       # unsorted
    assert b'sorted' in lib.flow_last_error()
    assert cum(2, ints(1, 2, 3), 1, 3, fake, fake, None) == 2       # first != 0
    assert cum(2, ints(0, 2, 4), 1, 3, fake, fake, None) == 2       # last
    assert cum(1, ints(0, 3), 1, 3, None, fake, None) == 2
    assert cum(1, ints(0, 3), 1, 3, fake, None, None) == 2
    assert b'pointers' in lib.flow_last_error()
    # flow_form_facet_values: no mesh, no form
    val = lib.flow_form_facet_values
    assert val(None, None, 0, None, None, None, None, None, None, None) == 2
