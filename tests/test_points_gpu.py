# -*- coding: utf-8 -*-
'''
Point evaluation on the HIP path (flow_amd/fem/points.py; csrc/
form_kernels.hip: locate_points_kernel, form_points_kernel): the GPU's
point location against the numpy brute force of tests/point_reference.py,
P_k-exact fields, a numpy evaluator, determinism, points outside the mesh,
the refusals, all 2.19 M centroids of the bench mesh, KarmanProblem's
pressure_difference(), and the pressure drop of the DFG 2D-1 benchmark
(Schaefer & Turek 1996, Re = 20) against its published value.
'''
import time

import numpy
import pytest
import torch

from flow_amd import device, fem, karman, stokes
from flow_amd.fem import (
    Probes, FacetNormal, SpatialCoordinate, sqrt, dot, grad, curl,
    )
from flow_amd.fem.mesh import rectangle_with_fitted_hole
import flow_amd.navier_stokes as navsto

import point_reference as ref

pytestmark = pytest.mark.gpu

CHANNEL = (0.0, 0.6, -0.07, 0.07)


def _meshes():
    return [fem.UnitSquareMesh(12, 9),
            fem.karman_channel(60, 14, fitted=True),
            fem.karman_channel_graded(lcar=1.0e-2)]


def _interpolate(V, funcs):
    u = fem.Function(V)
    xy = V.layout.dof_coords
    u.set_array(numpy.concatenate([f(xy[:, 0], xy[:, 1]) for f in funcs]))
    return u


def _q(x, y):
    return 1.0 + 2.0 * x - 3.0 * y + 0.5 * x * x + x * y - 2.0 * y * y


def _q2(x, y):
    return -0.5 + x - y + 3.0 * x * x - 2.0 * x * y + y * y


@pytest.mark.parametrize('k', range(3))
def test_location_against_brute_force(hip, k):
    mesh = _meshes()[k]
    sets = [ref.random_points(mesh, 20000, seed=k), mesh.points,
            ref.edge_midpoints(mesh)]
    if k:
        obst = ref.obstacle_vertices(mesh, CHANNEL)
        assert len(obst) >= 12
        sets.append(obst)
    for pts in sets:
        probes = Probes(mesh, pts)
        want = ref.locate(mesh, pts)
        assert probes.cells.dtype == numpy.int32
        assert numpy.array_equal(probes.cells, want)
        assert numpy.array_equal(probes.found, want >= 0)
        # the stored barycentric coordinates put the point where it is
        x = probes(SpatialCoordinate(mesh))
        f = probes.found
        scale = numpy.abs(mesh.points).max()
        assert numpy.abs(x[f] - pts[f]).max() <= 1e-14 * scale
        assert numpy.isnan(x[~f]).all()
    # random points: inside, in the hole and outside all occur
    cells = Probes(mesh, sets[0]).cells
    assert (cells >= 0).sum() > 1000 and (cells < 0).sum() > 100


@pytest.mark.parametrize('k', range(3))
def test_exact_fields(hip, k):
    mesh = _meshes()[k]
    P1 = fem.FunctionSpace(mesh, 'CG', 1)
    P2 = fem.FunctionSpace(mesh, 'CG', 2)
    W = fem.VectorFunctionSpace(mesh, 'CG', 2)
    q = _interpolate(P2, [_q])
    u = _interpolate(W, [_q, _q2])
    lin = _interpolate(P1, [lambda x, y: 3.0 + x - 2.0 * y])
    pts = ref.random_points(mesh, 4000, seed=10 + k, margin=0.0)
    probes = Probes(mesh, pts)
    f = probes.found
    x, y = pts[f, 0], pts[f, 1]

    def close(got, want):
        scale = numpy.abs(want).max()
        assert numpy.abs(got[f] - want).max() <= 1e-12 * scale

    close(probes(q), _q(x, y))
    close(probes(u), numpy.stack([_q(x, y), _q2(x, y)], axis=1))
    close(probes(lin), 3.0 + x - 2.0 * y)
    close(probes(grad(q)), numpy.stack([2.0 + x + y, -3.0 + x - 4.0 * y],
                                       axis=1))
    # curl (u0, u1) = d u1/dx - d u0/dy
    close(probes(curl(u)), (6.0 * x - 2.0 * y + 1.0) - (-3.0 + x - 4.0 * y))
    assert probes(q).shape == (len(pts),) and probes(u).shape == (len(pts), 2)


def test_against_numpy_evaluator(hip):
    for mesh in _meshes()[1:]:
        W = fem.VectorFunctionSpace(mesh, 'CG', 2)
        P1 = fem.FunctionSpace(mesh, 'CG', 1)
        u = _interpolate(W, [lambda x, y: numpy.sin(20 * x) * y + 1.0,
                             lambda x, y: numpy.cos(30 * y) * x])
        p = _interpolate(P1, [lambda x, y: numpy.exp(x) * y + 2.0])
        pts = ref.random_points(mesh, 2000, seed=3, margin=0.0)
        probes = Probes(mesh, pts)
        f = probes.found
        cells = probes.cells[f]
        uu = ref.field_values(u, pts[f], cells)
        pp = ref.field_values(p, pts[f], cells)
        scale = numpy.abs(uu).max()
        assert numpy.abs(probes(u)[f] - uu.T).max() <= 1e-13 * scale
        assert numpy.abs(probes(sqrt(dot(u, u)))[f]
                         - numpy.sqrt((uu**2).sum(axis=0))).max() \
            <= 1e-13 * scale
        assert numpy.abs(probes(p)[f] - pp[0]).max() \
            <= 1e-13 * numpy.abs(pp).max()
        # Constants travel with every call
        c = fem.Constant(2.0)
        a = probes(c * p)
        c.assign(3.0)
        assert numpy.abs(probes(c * p)[f] - 1.5 * a[f]).max() \
            <= 1e-14 * numpy.abs(a[f]).max()


def test_determinism(hip):
    mesh = fem.karman_channel_graded(lcar=1.0e-2)
    W = fem.VectorFunctionSpace(mesh, 'CG', 2)
    u = _interpolate(W, [lambda x, y: numpy.sin(20 * x) * y,
                         lambda x, y: numpy.cos(30 * y) * x])
    pts = numpy.concatenate([ref.random_points(mesh, 3000, seed=5),
                             mesh.points, ref.edge_midpoints(mesh)])
    probes = Probes(mesh, pts)
    expr = sqrt(dot(u, u)) + grad(u)[0, 1]
    a, b = probes(expr), probes(expr)
    assert a.tobytes() == b.tobytes()
    perm = numpy.random.RandomState(1).permutation(len(pts))
    other = Probes(mesh, pts[perm])
    assert numpy.array_equal(other.cells, probes.cells[perm])
    assert other(expr).tobytes() == a[perm].tobytes()
    assert other(u).tobytes() == probes(u)[perm].tobytes()
    # one point at a time: u(x) is the probes' entry, bit for bit
    vu = probes(u)
    p = fem.Function(fem.FunctionSpace(mesh, 'CG', 1))
    p.set_array(numpy.sin(7 * mesh.points[:, 0]) + mesh.points[:, 1])
    vp = probes(p)
    for i in numpy.nonzero(probes.found)[0][:20]:
        x, y = pts[i]
        assert u(x, y).tobytes() == vu[i].tobytes()
        assert isinstance(p(x, y), float)
        assert p(x, y) == vp[i]
        assert p(fem.Point(x, y)) == vp[i]
        assert p((x, y)) == vp[i]
        assert p(numpy.array([x, y])) == vp[i]
    # evaluate(): the device tensor, also into a given one
    out = torch.empty((2, len(pts)), dtype=torch.float64, device=device.get())
    got = probes.evaluate(u, out=out)
    assert got is out
    assert out.cpu().numpy().T.tobytes() == vu.tobytes()
    with pytest.raises(ValueError, match='shape'):
        probes.evaluate(u[0], out=out)


def test_outside_and_refusals(hip):
    mesh = fem.karman_channel(60, 14, fitted=True)
    W = fem.VectorFunctionSpace(mesh, 'CG', 2)
    P = fem.FunctionSpace(mesh, 'CG', 1)
    u, p = fem.Function(W), fem.Function(P)
    cx, cy, r = mesh.hole
    outside = [(-0.1, 0.0), (0.7, 0.0), (0.3, 0.2), (cx, cy), (numpy.nan, 0.0)]
    probes = Probes(mesh, outside + [(0.3, 0.0)])
    assert probes.cells[:5].tolist() == [-1] * 5 and probes.cells[5] >= 0
    v = probes(u)
    assert numpy.isnan(v[:5]).all() and not numpy.isnan(v[5]).any()
    assert numpy.isnan(probes(p)[:5]).all()
    for x in outside[:4]:
        with pytest.raises(RuntimeError, match='Unable to evaluate function'):
            p(*x)
        with pytest.raises(RuntimeError, match='Unable to evaluate function'):
            u(x)
    with pytest.raises(ValueError, match='Expression'):
        probes(fem.Expression('x[0]', degree=1) * p)
    with pytest.raises(ValueError, match='FacetNormal'):
        probes(dot(u, FacetNormal(mesh)))
    with pytest.raises(ValueError, match='components'):
        probes(grad(u))
    other = fem.Function(fem.FunctionSpace(fem.UnitSquareMesh(3, 3), 'CG', 1))
    with pytest.raises(ValueError, match='mesh'):
        probes(other)
    # no points at all
    empty = Probes(mesh, numpy.zeros((0, 2)))
    assert empty(p).shape == (0,) and empty(u).shape == (0, 2)


def test_bench_mesh_centroids(hip):
    '''The bench mesh of KarmanProblem(2182, 509): centroid i lies in cell
    i, for all 2.19 M cells.'''
    mesh = fem.karman_channel(2182, 509, fitted=True)
    cen = mesh.points[mesh.cell_vertices].mean(axis=1)
    t0 = time.time()
    probes = Probes(mesh, cen)
    print('located %d centroids in %.2f s (grid and upload included)'
          % (len(cen), time.time() - t0))
    assert numpy.array_equal(probes.cells,
                             numpy.arange(mesh.num_cells(), dtype=numpy.int32))


def test_karman_pressure_difference(hip):
    problem = karman.KarmanProblem(60, 14)
    problem.set_initial_stokes()
    problem.step()
    cx, cy, r = problem.mesh.hole
    dp = problem.pressure_difference()
    p = problem.p0
    assert dp == p(cx - r, cy) - p(cx + r, cy)
    # the two points are vertices: their P1 dofs
    P = problem.P
    xy = P.layout.dof_coords
    vals = p.array()
    want = []
    for x in (cx - r, cx + r):
        i = numpy.argmin(numpy.hypot(xy[:, 0] - x, xy[:, 1] - cy))
        assert numpy.hypot(xy[i, 0] - x, xy[i, 1] - cy) < 1e-15
        want.append(vals[i])
    assert abs(dp - (want[0] - want[1])) <= 1e-14 * numpy.abs(vals).max()
    assert problem.pressure_difference() == dp          # cached probes
    with pytest.raises(ValueError, match='fitted'):
        karman.KarmanProblem(60, 14, fitted=False).pressure_difference()


# -- DFG 2D-1 --------------------------------------------------------------------
DFG_H = 0.41
DFG_UMAX = 0.3
DFG_DP = 0.11752016697


class _DfgWalls(fem.SubDomain):
    def inside(self, x, on_boundary):
        return on_boundary & ((x[1] < 1e-12) | (x[1] > DFG_H - 1e-12))


class _DfgInflow(fem.SubDomain):
    def inside(self, x, on_boundary):
        return on_boundary & (x[0] < 1e-12)


class _DfgOutflow(fem.SubDomain):
    def inside(self, x, on_boundary):
        return on_boundary & (x[0] > 2.2 - 1e-12)


class _DfgCylinder(fem.SubDomain):
    def inside(self, x, on_boundary):
        return on_boundary & (1e-12 < x[0]) & (x[0] < 2.2 - 1e-12) \
            & (1e-12 < x[1]) & (x[1] < DFG_H - 1e-12)


def dfg_steady(nx, ny, dt, max_steps=6000, rtol=1.0e-10):
    '''Steady DFG 2D-1 (the setup of test_facet_forms_gpu.dfg_coefficients):
    Stokes start, IPCS steps until the relative change of the velocity per
    step is below rtol.  Returns (p0, steps, last change, mesh).'''
    mesh = rectangle_with_fitted_hole(0.0, 2.2, 0.0, DFG_H, (0.2, 0.2), 0.05,
                                      nx, ny)
    rho, mu = 1.0, 1.0e-3
    W = fem.VectorFunctionSpace(mesh, 'CG', 2)
    P = fem.FunctionSpace(mesh, 'CG', 1)
    inflow = fem.Expression(
        ('4.0*%r*x[1]*(%r - x[1])/(%r*%r)' % (DFG_UMAX, DFG_H, DFG_H, DFG_H),
         '0.0'), degree=2)

    def velocity_bcs(V):
        return [fem.DirichletBC(V, (0.0, 0.0), _DfgWalls()),
                fem.DirichletBC(V, (0.0, 0.0), _DfgCylinder()),
                fem.DirichletBC(V, inflow, _DfgInflow())]

    WP = fem.FunctionSpace(mesh, fem.VectorElement('Lagrange', 'triangle', 2)
                           * fem.FiniteElement('Lagrange', 'triangle', 1))
    us, ps = stokes.solve(WP, velocity_bcs(WP.sub(0)), fem.Constant(mu),
                          f=fem.Constant((0.0, 0.0)), verbose=False)
    u0, p0 = fem.Function(W), fem.Function(P)
    fem.ops.copy(u0.data, us.data)
    fem.ops.copy(p0.data, ps.data)
    u_bcs = velocity_bcs(W)
    p_bcs = [fem.DirichletBC(P, 0.0, _DfgOutflow())]
    method = navsto.IPCS()
    zero = fem.Constant((0.0, 0.0))
    change = numpy.inf
    steps = 0
    while change >= rtol and steps < max_steps:
        u1, p1 = method.step(fem.Constant(dt), {0: u0}, p0, u_bcs, p_bcs,
                             fem.Constant(rho), fem.Constant(mu),
                             f={0: zero, 1: zero}, verbose=False, tol=1.0e-12)
        change = float((u1.data - u0.data).norm() / u1.data.norm())
        u0.assign(u1)
        p0.assign(p1)
        steps += 1
    return p0, steps, change, mesh


# 440 x 82, dt = 0.02 (the mesh and step of the drag / lift test).  Measured
# there: dp = 0.117242 (published 0.11752016697: -0.24 %), 1597 steps, 6 s.
def test_dfg_2d1_pressure_drop(hip):
    t0 = time.time()
    p0, steps, change, mesh = dfg_steady(440, 82, 0.02)
    front, back = (0.15, 0.2), (0.25, 0.2)
    probes = Probes(mesh, [front, back])
    vals = probes(p0)
    dp = vals[0] - vals[1]
    print('DFG 2D-1 on %d cells: dp = %.6f (%.3f %%), %d steps, change %.1e, '
          '%.1f s' % (mesh.num_cells(), dp, 100 * (dp / DFG_DP - 1), steps,
                      change, time.time() - t0))
    assert change < 1.0e-10
    # both points are vertices: the probes give their P1 dofs
    xy = p0.function_space().layout.dof_coords
    dofs = p0.array()
    for k, (x, y) in enumerate((front, back)):
        i = numpy.argmin(numpy.hypot(xy[:, 0] - x, xy[:, 1] - y))
        assert numpy.hypot(xy[i, 0] - x, xy[i, 1] - y) < 1e-15
        assert abs(vals[k] - dofs[i]) <= 1e-14
    # the circle the mesh fitted is the benchmark's: the same two points
    cx, cy, r = mesh.hole
    assert abs(cx - r - front[0]) < 1e-15 and abs(cx + r - back[0]) < 1e-15
    assert abs(dp / DFG_DP - 1) < 0.02
