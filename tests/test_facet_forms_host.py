# -*- coding: utf-8 -*-
'''Exterior-facet integrals (`ds`, FacetNormal, facet markers) on the host:
names, the facet predicate SubDomain.mark shares with DirichletBC, the
Gauss-Legendre facet rule, degree estimation, where the normal is legal, the
register programs, form sums, and the numpy facet evaluator of
tests/facet_reference.py pinned by closed forms.  No GPU needed.'''
import os
import sys

import numpy
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from flow_amd import fem, karman, parallel, _hip, device     # noqa: E402
from flow_amd.fem import (                                   # noqa: E402
    assemble, dx, ds, Measure, FacetNormal, MeshFunction, FacetFunction,
    SpatialCoordinate, as_vector, sqrt, dot, grad, div, forms, reference,
    )
import facet_reference as fac                                # noqa: E402


def test_names_and_no_cpu_fallback():
    for name in ('ds', 'Measure', 'FacetNormal', 'MeshFunction',
                 'FacetFunction'):
        assert hasattr(fem, name), name
    assert forms.OPS['normal'] == 18 and forms.OPS['out'] == 17
    if device.on_gpu():
        pytest.skip('GPU present')
    mesh = fem.UnitSquareMesh(2, 2)
    with pytest.raises(_hip.HipError):
        assemble(1.0 * ds(mesh))


def test_strips_refused(monkeypatch):
    mesh = fem.UnitSquareMesh(2, 2)
    monkeypatch.setattr(parallel, 'active', lambda: True)
    with pytest.raises(NotImplementedError):
        assemble(1.0 * ds(mesh))
    with pytest.raises(NotImplementedError):
        assemble(1.0 * dx(mesh) + 1.0 * ds(mesh))


def _boundaries():
    return [karman.LeftBoundary(), karman.RightBoundary(),
            karman.LowerBoundary(), karman.UpperBoundary(),
            karman.ObstacleBoundary()]


def test_mark_selects_the_facets_of_dirichlet_bc():
    mesh = fem.karman_channel(60, 14, fitted=True)
    P2 = fem.FunctionSpace(mesh, 'CG', 2)
    lay = P2.layout
    markers = MeshFunction('size_t', mesh, 1, value=0)
    assert markers.size() == mesh.num_edges()
    seen = numpy.zeros(len(mesh.bfacets), dtype=int)
    for k, sub in enumerate(_boundaries(), start=1):
        m = MeshFunction('size_t', mesh, 1, 0)
        sub.mark(m, k)
        sub.mark(markers, k)
        edges = numpy.nonzero(m.array() == k)[0]
        # only exterior facets (on_boundary is False inside)
        assert numpy.isin(edges, mesh.bfacets).all()
        assert len(edges) > 0
        dofs = numpy.unique(numpy.concatenate([
            lay.vertex_dofs[mesh.edges[edges].ravel()], lay.edge_dofs[edges]]))
        bc = fem.DirichletBC(P2, 0.0, sub)
        assert numpy.array_equal(dofs, bc._scalar_dofs()), k
        seen += numpy.isin(mesh.bfacets, edges)
    # the five parts cover the boundary once (corners: one facet each)
    assert (seen == 1).all()
    vals = markers.array()[mesh.bfacets]
    assert set(vals.tolist()) == {1, 2, 3, 4, 5}
    # interior edges keep their value
    interior = numpy.setdiff1d(numpy.arange(mesh.num_edges()), mesh.bfacets)
    assert (markers.array()[interior] == 0).all()
    # a predicate that ignores on_boundary marks interior edges too
    class Left(fem.SubDomain):
        def inside(self, x, on_boundary):
            return x[0] < 0.05
    m = FacetFunction('size_t', mesh)
    Left().mark(m, 7)
    assert (m.array()[interior] == 7).any()


def test_mesh_function():
    mesh = fem.UnitSquareMesh(3, 3)
    m = MeshFunction('size_t', mesh, 1, value=2)
    assert (m.array() == 2).all() and m.array().dtype == numpy.uintp
    v = m.version
    with pytest.raises(ValueError):
        m.array()[0] = 5                    # read-only view
    m.set_all(4)
    assert (m.array() == 4).all() and m.version > v
    v = m.version
    m[3] = 1
    assert m[3] == 1 and m.version > v
    f = FacetFunction('size_t', mesh, value=1)
    assert isinstance(f, MeshFunction) and (f.array() == 1).all()
    with pytest.raises(NotImplementedError):
        MeshFunction('size_t', mesh, 2)


def test_line_rule():
    for q in range(0, 31):
        s, w = reference.line_rule(q)
        assert len(s) == q // 2 + 1
        assert ((0 < s) & (s < 1)).all()
        for k in range(q + 1):
            assert abs(numpy.dot(w, s**k) - 1.0 / (k + 1)) < 1e-14, (q, k)
    # not exact one degree above (odd q: 2n - 1 = q)
    s, w = reference.line_rule(3)
    assert abs(numpy.dot(w, s**4) - 0.2) > 1e-6
    # the facet layout: 3 nq rows, facet i opposite vertex i, weights sum 1
    rule = reference.facet_rule(4)
    nq = len(reference.line_rule(4)[0])
    assert rule.shape == (3 * nq, 3)
    xi, eta = rule[:, 0], rule[:, 1]
    assert numpy.allclose(xi[:nq] + eta[:nq], 1.0)         # facet 0
    assert numpy.allclose(xi[nq:2 * nq], 0.0)               # facet 1
    assert numpy.allclose(eta[2 * nq:], 0.0)                # facet 2
    for f in range(3):
        assert abs(rule[f * nq:(f + 1) * nq, 2].sum() - 1.0) < 1e-15


def test_measures_and_degrees():
    mesh = fem.UnitSquareMesh(2, 2)
    P1 = fem.FunctionSpace(mesh, 'CG', 1)
    P2 = fem.FunctionSpace(mesh, 'CG', 2)
    p, th = fem.Function(P1), fem.Function(P2)
    n = FacetNormal(mesh)
    x = SpatialCoordinate(mesh)
    markers = MeshFunction('size_t', mesh, 1, 0)
    assert n.shape == (2,) and n.deg == 0
    assert (th * n[0] * ds).degree() == 2
    assert (p * th * n[1] * ds).degree() == 3
    assert (dot(grad(th), n) * ds).degree() == 1
    assert (x[0] * n[0] * ds).degree() == 1
    assert (th * ds(metadata={'quadrature_degree': 7})).degree() == 7
    assert (th * ds(degree=5)).degree() == 5
    # the spellings
    for m in (ds(mesh), ds(domain=mesh)):
        f = 1.0 * m
        assert f.mesh is mesh and f.integral_type == 'exterior_facet'
        assert f.subdomain_id == 'everywhere'
    assert (th * ds(1)).subdomain_id == 1
    assert (th * ds(subdomain_id=2)).subdomain_id == 2
    dsm = Measure('ds', domain=mesh, subdomain_data=markers)
    f = th * dsm(3, degree=4)
    assert (f.subdomain_id, f.subdomain_data, f.mesh, f.degree()) == \
        (3, markers, mesh, 4)
    assert (1.0 * dsm).subdomain_id == 'everywhere'
    assert (1.0 * dsm(1)).mesh is mesh      # the mesh comes from the markers
    # dx unchanged
    f = th * dx
    assert f.integral_type == 'cell' and f.degree() == 2
    assert (1.0 * dx(mesh)).mesh is mesh
    with pytest.raises(NotImplementedError):
        dx(1)
    with pytest.raises(NotImplementedError):
        Measure('dS')
    other = fem.UnitSquareMesh(3, 3)
    with pytest.raises(ValueError, match='two different meshes'):
        p * Measure('ds', subdomain_data=MeshFunction('size_t', other, 1))


def test_normal_only_on_facets():
    mesh = fem.UnitSquareMesh(2, 2)
    P1 = fem.FunctionSpace(mesh, 'CG', 1)
    W = fem.VectorFunctionSpace(mesh, 'CG', 2)
    u = fem.Function(W)
    n = FacetNormal(mesh)
    with pytest.raises(ValueError, match='FacetNormal'):
        n[0] * dx
    with pytest.raises(ValueError, match='FacetNormal'):
        sqrt(dot(u, n)**2 + 1.0) * dx(mesh)
    with pytest.raises(ValueError, match='FacetNormal'):
        fem.project(n[0], P1)
    with pytest.raises(ValueError, match='FacetNormal'):
        fem.project(as_vector([n[1], u[0]]), fem.VectorFunctionSpace(
            mesh, 'CG', 1))
    with pytest.raises(ValueError, match='FacetNormal'):
        forms.Program([(u[0] * n[0]).comps])
    with pytest.raises(ValueError, match='scalar integrands'):
        n * ds
    with pytest.raises(ValueError, match='scalar integrands'):
        u * ds(mesh)
    # the normal is constant on a facet: its derivatives vanish
    assert grad(n[0]).comps == [forms.ZERO, forms.ZERO]


def test_programs():
    mesh = fem.UnitSquareMesh(2, 2)
    W = fem.VectorFunctionSpace(mesh, 'CG', 2)
    u = fem.Function(W)
    n = FacetNormal(mesh)
    ops = forms.OPS
    prog = forms.Program([dot(u, n).comps], facet=True)
    code = [c[0] for c in prog.code]
    assert code.count(ops['normal']) == 2
    assert sorted(c[2] for c in prog.code if c[0] == ops['normal']) == [0, 1]
    for f in (div(u), dot(u, u), sqrt(u[0]**2 + 1.0)):
        for facet in (False, True):
            code = [c[0] for c in forms.Program([f.comps], facet=facet).code]
            assert ops['normal'] not in code


def test_form_sums():
    mesh = fem.UnitSquareMesh(4, 4)
    x = SpatialCoordinate(mesh)
    a, b, c = x[0] * dx, 2.0 * ds(mesh), x[1] * ds(3)
    s = a + b - c
    assert isinstance(s, forms.FormSum) and isinstance(s, forms.Form)
    assert [(sg, f) for sg, f in s.terms()] == [(1.0, a), (1.0, b), (-1.0, c)]
    assert [sg for sg, _ in (-(a - b)).terms()] == [-1.0, 1.0]
    assert [f for _, f in sum([a, b, c]).terms()] == [a, b, c]
    with pytest.raises(TypeError):
        s.degree()
    with pytest.raises(TypeError):
        a + 1.0


def test_facet_evaluator_closed_forms():
    '''The evaluator on a rectangle: perimeter, int x n_x ds = area, the
    divergence theorem for a P2 field, the parts of a marked boundary.'''
    x0, x1, y0, y1 = 0.5, 2.0, -1.0, 1.5
    mesh = fem.RectangleMesh(fem.Point(x0, y0), fem.Point(x1, y1), 5, 4)
    X = SpatialCoordinate(mesh)
    n = FacetNormal(mesh)
    per = 2 * (x1 - x0) + 2 * (y1 - y0)
    area = (x1 - x0) * (y1 - y0)
    assert abs(fac.functional(1.0 * ds(mesh)) - per) < 1e-14 * per
    assert abs(fac.functional(X[0] * n[0] * ds(mesh)) - area) < 1e-13
    assert abs(fac.functional(X[1] * n[1] * ds(mesh)) - area) < 1e-13
    assert abs(fac.functional(X[0] * n[1] * ds(mesh))) < 1e-13
    W = fem.VectorFunctionSpace(mesh, 'CG', 2)
    u = fem.Function(W)
    xy = W.layout.dof_coords
    u.set_array(numpy.concatenate([xy[:, 0]**2 + xy[:, 0] * xy[:, 1],
                                   xy[:, 1]**2 - 3 * xy[:, 0]]))
    flux = fac.functional(dot(u, n) * ds)
    assert abs(flux - fac.functional(div(u) * dx)) < 1e-12
    # marked: the left side x = x0
    class Left(fem.SubDomain):
        def inside(self, x, on_boundary):
            return on_boundary & (x[0] < x0 + 1e-12)
    m = MeshFunction('size_t', mesh, 1, 0)
    Left().mark(m, 1)
    dsm = Measure('ds', domain=mesh, subdomain_data=m)
    assert abs(fac.functional(1.0 * dsm(1)) - (y1 - y0)) < 1e-14
    assert abs(fac.functional(n[0] * dsm(1)) + (y1 - y0)) < 1e-14
    assert fac.functional(1.0 * dsm(9)) == 0.0
    got = fac.functional(1.0 * dsm(1) + 1.0 * dsm(0) - 0.5 * X[0] * dx)
    want = per - 0.5 * 0.5 * (x0 + x1) * area
    assert abs(got - want) < 1e-13
