# -*- coding: utf-8 -*-
'''
Point evaluation without a GPU (flow_amd/fem/points.py): the bucket grid's
invariants -- every cell listed in every bucket its bounding box overlaps,
each bucket ascending, the brute-force owner of random points among their
bucket's candidates --, the fitted hole a mesh records, and the host-side
refusals of the point compiler.
'''
import numpy
import pytest

from flow_amd import fem
from flow_amd.fem import forms, points, FacetNormal, grad, sqrt, dot
from flow_amd.fem.mesh import rectangle_with_fitted_hole

import point_reference as ref


def _meshes():
    return [fem.UnitSquareMesh(12, 9),
            fem.karman_channel(60, 14, fitted=True),
            fem.karman_channel_graded(lcar=1.0e-2)]


@pytest.mark.parametrize('k', range(3))
def test_grid_invariants(k):
    mesh = _meshes()[k]
    g = points.PointGrid(mesh)
    nb = g.nx * g.ny
    assert g.start[0] == 0 and g.start[-1] == len(g.cells)
    assert (numpy.diff(g.start) >= 0).all()
    # each bucket ascending (strictly: a cell is listed once per bucket)
    per = numpy.diff(g.start)
    bucket_of = numpy.repeat(numpy.arange(nb), per)
    same = bucket_of[1:] == bucket_of[:-1]
    assert (numpy.diff(g.cells.astype(numpy.int64))[same] > 0).all()
    # every cell in every bucket its (unpadded) bounding box overlaps
    v = mesh.points[mesh.cell_vertices]
    i0, j0 = g.bucket_xy(v.min(axis=1))
    i1, j1 = g.bucket_xy(v.max(axis=1))
    listed = set(zip(bucket_of.tolist(), g.cells.tolist()))
    for c in range(mesh.num_cells()):
        for iy in range(j0[c], j1[c] + 1):
            for ix in range(i0[c], i1[c] + 1):
                assert (iy * g.nx + ix, c) in listed, (c, ix, iy)
    # the brute-force owner of random points is among their candidates
    pts = ref.random_points(mesh, 10000, seed=k)
    owner = ref.locate(mesh, pts)
    assert (owner >= 0).sum() > 5000
    b = g.bucket(pts)
    for i in numpy.nonzero(owner >= 0)[0]:
        assert owner[i] in g.candidates(b[i]), i
    # the cached grid
    assert points.point_grid(mesh) is points.point_grid(mesh)
    mean, most = g.stats()
    assert 1.0 <= mean <= 12.0 and most <= 40


def test_fitted_hole_is_recorded():
    mesh = fem.karman_channel(60, 14, fitted=True)
    hx, hy = 0.6 / 60, 0.14 / 14
    ic, jc = int(round(0.1 / hx)), int(round((0.01 + 0.07) / hy))
    assert mesh.hole == (0.0 + ic * hx, -0.07 + jc * hy, 0.02)
    cx, cy, r = mesh.hole
    # the front and back points of the circle are mesh vertices
    for x in (cx - r, cx + r):
        d = numpy.hypot(mesh.points[:, 0] - x, mesh.points[:, 1] - cy).min()
        assert d < 1e-15
    assert fem.karman_channel(60, 14).hole is None             # staircase
    assert fem.UnitSquareMesh(3, 3).hole is None
    assert mesh.reordered().hole == mesh.hole
    dfg = rectangle_with_fitted_hole(0.0, 2.2, 0.0, 0.41, (0.2, 0.2), 0.05,
                                     440, 82)
    assert abs(dfg.hole[0] - 0.2) < 1e-15 and abs(dfg.hole[1] - 0.2) < 1e-15
    assert dfg.hole[2] == 0.05


def test_point_programs():
    mesh = fem.UnitSquareMesh(4, 4)
    W = fem.VectorFunctionSpace(mesh, 'CG', 2)
    P = fem.FunctionSpace(mesh, 'CG', 1)
    u, p = fem.Function(W), fem.Function(P)
    x = fem.SpatialCoordinate(mesh)
    assert forms.point_program(p).nout == 1
    assert forms.point_program(u).nout == 2
    assert forms.point_program(grad(p)).nout == 2
    assert forms.point_program(sqrt(dot(u, u)) + x[0]).nout == 1
    assert forms.point_program(grad(u)[0]).nout == 2
    ex = fem.Expression('x[0]', degree=1)
    with pytest.raises(ValueError, match='Expression'):
        forms.point_program(ex * p)
    with pytest.raises(ValueError, match='FacetNormal'):
        forms.point_program(dot(u, FacetNormal(mesh)))
    with pytest.raises(ValueError, match='components'):
        forms.point_program(grad(u))
    # integrals still compile as before
    assert forms.Program([(ex * p).comps]).nout == 1


def test_point_arguments():
    assert points.as_points([(0.0, 1.0), (2.0, 3.0)]).shape == (2, 2)
    assert points.as_points([fem.Point(0.5, 0.5)]).tolist() == [[0.5, 0.5]]
    assert points.as_points(numpy.zeros((0, 2))).shape == (0, 2)
    with pytest.raises(ValueError):
        points.as_points([1.0, 2.0, 3.0])
    u = fem.Function(fem.FunctionSpace(fem.UnitSquareMesh(2, 2), 'CG', 1))
    with pytest.raises(TypeError):
        u(0.1, 0.2, 0.3)
    with pytest.raises(ValueError):
        u((0.1, 0.2, 0.3))


def test_reference_rule():
    '''The brute force of point_reference: vertices and edge midpoints go to
    their lowest-index incident cell.'''
    mesh = fem.UnitSquareMesh(5, 4)
    owner = ref.locate(mesh, mesh.points)
    cv = mesh.cell_vertices
    for v in range(mesh.num_vertices()):
        assert owner[v] == numpy.nonzero((cv == v).any(axis=1))[0].min()
    mids = ref.edge_midpoints(mesh)
    owner = ref.locate(mesh, mids)
    for e, (a, b) in enumerate(mesh.edges):
        incident = numpy.nonzero((cv == a).any(axis=1) & (cv == b).any(axis=1))[0]
        assert owner[e] == incident.min()
    assert (ref.locate(mesh, [[-0.5, 0.5], [1.5, 0.5]]) == -1).all()
