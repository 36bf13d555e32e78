# -*- coding: utf-8 -*-
'''
assemble(f*ds) on the HIP path (flow_amd/fem/forms.py,
csrc/form_kernels.hip: form_facet_kernel): boundary lengths, marked parts,
the divergence theorem, the numpy facet evaluator of tests/facet_reference.py,
plane Poiseuille flow (exact in P2-P1), determinism and the facet-list
cache, KarmanProblem.forces(), and the drag and lift of the DFG 2D-1
benchmark (Schaefer & Turek 1996, Re = 20) against its published values.
'''
import time

import numpy
import pytest

from flow_amd import fem, karman, stokes
from flow_amd.fem import (
    assemble, dx, ds, Measure, FacetNormal, MeshFunction, SpatialCoordinate,
    sqrt, exp, sin, dot, inner, grad, div, forms,
    )
from flow_amd.fem.mesh import rectangle_with_fitted_hole
import flow_amd.navier_stokes as navsto

import facet_reference as fac

pytestmark = pytest.mark.gpu


def _rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


def _meshes():
    return [fem.UnitSquareMesh(12, 9),
            fem.karman_channel(60, 14, fitted=True),
            fem.karman_channel_graded(lcar=1.0e-2)]


def _boundary_length(mesh):
    ev = mesh.edges[mesh.bfacets]
    d = mesh.points[ev[:, 1]] - mesh.points[ev[:, 0]]
    return float(numpy.hypot(d[:, 0], d[:, 1]).sum())


def _p2_field(W, funcs):
    u = fem.Function(W)
    xy = W.layout.dof_coords
    u.set_array(numpy.concatenate([f(xy[:, 0], xy[:, 1]) for f in funcs]))
    return u


def _channel_markers(mesh):
    m = MeshFunction('size_t', mesh, 1, 0)
    for k, sub in enumerate([karman.LeftBoundary(), karman.RightBoundary(),
                             karman.LowerBoundary(), karman.UpperBoundary(),
                             karman.ObstacleBoundary()], start=1):
        sub.mark(m, k)
    return m


def test_boundary_length(hip):
    for mesh in _meshes():
        per = _boundary_length(mesh)
        assert _rel(assemble(1.0 * ds(mesh)), per) < 1e-14
        assert _rel(assemble(fem.Constant(1.0) * ds(domain=mesh)), per) < 1e-14


def test_marked_parts(hip):
    for mesh in _meshes()[1:]:
        per = _boundary_length(mesh)
        m = _channel_markers(mesh)
        dsm = Measure('ds', domain=mesh, subdomain_data=m)
        parts = [assemble(1.0 * dsm(k)) for k in range(1, 6)]
        assert _rel(sum(parts), per) < 1e-13
        total = assemble(1.0 * dsm(1) + 1.0 * dsm(2) + 1.0 * dsm(3)
                         + 1.0 * dsm(4) + 1.0 * dsm(5))
        assert _rel(total, per) < 1e-13
        assert _rel(parts[0], 0.14) < 1e-14                     # inflow
        assert _rel(parts[1], 0.14) < 1e-14                     # outflow
        assert _rel(parts[2], 0.6) < 1e-14                      # lower wall
        # the obstacle: a polygon inscribed in the circle of radius 0.02
        assert 0.0 < 2 * numpy.pi * 0.02 - parts[4] < 2e-3
        assert assemble(1.0 * dsm(6)) == 0.0                    # unused id
        # dx and ds in one sum
        area = mesh.cell_areas().sum()
        assert _rel(assemble(2.0 * dx(mesh) - 1.0 * dsm(1)),
                    2 * area - 0.14) < 1e-13


def test_divergence_theorem(hip):
    for mesh in _meshes():
        W = fem.VectorFunctionSpace(mesh, 'CG', 2)
        F = _p2_field(W, [lambda x, y: numpy.sin(20 * x) * y + x * x,
                          lambda x, y: numpy.cos(30 * y) * x - y])
        n = FacetNormal(mesh)
        vol = assemble(div(F) * dx)
        flux = assemble(dot(F, n) * ds)
        scale = assemble(sqrt(dot(F, F)) * ds)
        assert abs(vol - flux) < 1e-12 * scale
        x = SpatialCoordinate(mesh)
        area = mesh.cell_areas().sum()
        assert _rel(assemble(x[0] * n[0] * ds), area) < 1e-12
        assert _rel(assemble(x[1] * n[1] * ds(mesh)), area) < 1e-12
        assert abs(assemble(x[0] * n[1] * ds)) < 1e-12 * area


def test_against_facet_reference(hip):
    for mesh in _meshes()[1:]:
        P1 = fem.FunctionSpace(mesh, 'CG', 1)
        P2 = fem.FunctionSpace(mesh, 'CG', 2)
        W = fem.VectorFunctionSpace(mesh, 'CG', 2)
        u = _p2_field(W, [lambda x, y: numpy.sin(20 * x) * y + 1.0,
                          lambda x, y: numpy.cos(30 * y) * x])
        p = fem.interpolate(fem.Expression('exp(x[0])*x[1] + 2', degree=3), P1)
        th = fem.interpolate(fem.Expression('0.5 + x[0]*x[1]', degree=2), P2)
        X = SpatialCoordinate(mesh)
        n = FacetNormal(mesh)
        ex = fem.Expression('sin(40*x[0]) + x[1]', degree=4)
        ev = fem.Expression(('x[1]', 'x[0]*x[0]'), degree=2)
        c = fem.Constant(1.7)
        m = _channel_markers(mesh)
        dsm = Measure('ds', domain=mesh, subdomain_data=m)
        integrands = [
            inner(u, u), dot(u, n), p * n[0] - th * n[1],
            dot(grad(p), n) * th, sqrt(u[0]**2 + u[1]**2 + 1.0),
            dot(dot(grad(u), n), u), ex * u[0] + dot(ev, n),
            c * th**2 * X[0] * n[1], sin(X[1] * 30) * exp(th) + X[0],
            div(u) * p / (th + 1.0),
            ]
        for f in integrands:
            for measure in (ds, dsm(1), dsm(3), dsm(5), dsm(5, degree=6)):
                got = assemble(f * measure)
                want = fac.functional(f * measure)
                # (scale: the integral of |f|, at least the length of the
                # part: some integrands nearly vanish on some parts)
                scale = max(fac.functional(abs(f) * measure),
                            fac.functional(1.0 * measure(domain=mesh)))
                assert abs(got - want) <= 1e-12 * scale, \
                    (measure.subdomain_id, got, want)


def test_poiseuille(hip):
    '''u = (4 Um y (H - y) / H^2, 0), p = G (L - x) with G = 8 mu Um / H^2:
    P2 and P1 hold them exactly, so the traction integrals are exact.'''
    L, H, Um, mu = 2.0, 0.5, 1.5, 0.3
    G = 8 * mu * Um / H**2
    mesh = fem.RectangleMesh(fem.Point(0.0, 0.0), fem.Point(L, H), 16, 6)
    W = fem.VectorFunctionSpace(mesh, 'CG', 2)
    P = fem.FunctionSpace(mesh, 'CG', 1)
    u = _p2_field(W, [lambda x, y: 4 * Um * y * (H - y) / H**2,
                      lambda x, y: 0.0 * x])
    p = fem.Function(P)
    p.set_array(G * (L - P.layout.dof_coords[:, 0]))
    n = FacetNormal(mesh)
    gu = grad(u)

    def traction(a):
        return mu * ((gu[a, 0] + gu[0, a]) * n[0]
                     + (gu[a, 1] + gu[1, a]) * n[1]) - p * n[a]

    class Wall(fem.SubDomain):
        def inside(self, x, on_boundary):
            return on_boundary & ((x[1] < 1e-12) | (x[1] > H - 1e-12))

    m = MeshFunction('size_t', mesh, 1, 0)
    Wall().mark(m, 1)
    dsm = Measure('ds', domain=mesh, subdomain_data=m)
    # the force of the fluid on the two walls: 2 * mu * (4 Um / H) * L
    shear = -assemble(traction(0) * dsm(1))
    assert _rel(shear, 8 * mu * Um * L / H) < 1e-12
    assert abs(assemble(traction(1) * dsm(1))) < 1e-12 * G * L * H
    # div sigma = mu lap u - grad p = 0: no net force on the whole boundary
    # (scale: the pressure force on the inflow, G L H)
    for a in range(2):
        assert abs(assemble(traction(a) * ds)) < 1e-12 * G * L * H


def test_determinism_and_cache(hip):
    mesh = fem.karman_channel_graded(lcar=1.0e-2)
    W = fem.VectorFunctionSpace(mesh, 'CG', 2)
    u = _p2_field(W, [lambda x, y: numpy.sin(20 * x) * y,
                      lambda x, y: numpy.cos(30 * y) * x])
    n = FacetNormal(mesh)
    m = _channel_markers(mesh)
    dsm = Measure('ds', domain=mesh, subdomain_data=m)
    f = sqrt(inner(u, u) + 1.0) * dot(u, n) * dsm(5)
    vals = [assemble(f) for _ in range(3)]
    assert vals[0].hex() == vals[1].hex() == vals[2].hex()
    # a time loop re-assigns Constants: new values, the same facet lists
    lists = fem.ops.facet_lists(mesh, m, 5)
    c = fem.Constant(1.0)
    a1 = assemble(c * u[0] * dsm(5))
    c.assign(3.0)
    assert _rel(assemble(c * u[0] * dsm(5)), 3.0 * a1) < 1e-14
    again = fem.ops.facet_lists(mesh, m, 5)
    assert again[0] is lists[0] and again[1] is lists[1]
    # re-marking selects again
    obstacle = assemble(1.0 * dsm(5))
    m.set_all(0)
    assert assemble(1.0 * dsm(5)) == 0.0
    karman.ObstacleBoundary().mark(m, 5)
    assert assemble(1.0 * dsm(5)) == obstacle
    karman.LeftBoundary().mark(m, 5)
    assert _rel(assemble(1.0 * dsm(5)), obstacle + 0.14) < 1e-13


def test_karman_forces(hip):
    problem = karman.KarmanProblem(60, 14)
    problem.set_initial_stokes()
    got = problem.forces()
    mesh = problem.mesh
    m = MeshFunction('size_t', mesh, 1, 0)
    karman.ObstacleBoundary().mark(m, 1)
    dsm = Measure('ds', domain=mesh, subdomain_data=m)
    n = FacetNormal(mesh)
    gu = grad(problem.u0)
    mu, p = problem.mu, problem.p0
    want = []
    for a in range(2):
        t = mu * ((gu[a, 0] + gu[0, a]) * n[0]
                  + (gu[a, 1] + gu[1, a]) * n[1]) - p * n[a]
        want.append(-fac.functional(t * dsm(1)))
        scale = fac.functional(abs(t) * dsm(1))
        assert abs((got['drag'], got['lift'])[a] - want[a]) < 1e-12 * scale
    # Stokes flow past the cylinder: drag downstream
    assert got['drag'] > 0.0
    k = 2.0 / (problem.rho * karman.ENTRANCE_VELOCITY**2 * 0.04)
    assert _rel(got['c_drag'], k * got['drag']) < 1e-15
    assert _rel(got['c_lift'], k * got['lift']) < 1e-15
    # cached markers: the same numbers again
    again = problem.forces()
    assert again['drag'] == got['drag'] and again['lift'] == got['lift']


# -- DFG 2D-1 --------------------------------------------------------------------
DFG_H = 0.41
DFG_UMAX = 0.3
DFG_UMEAN = 0.2
DFG_D = 0.1
DFG_CD = 5.57953523
DFG_CL = 0.0106189


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


def dfg_coefficients(nx, ny, dt, max_steps=6000, rtol=1.0e-10, log=None):
    '''Steady DFG 2D-1: Stokes start, IPCS steps until the relative change
    of the velocity per step is below rtol.  Returns (c_D, c_L, steps,
    last change, mesh).'''
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
    markers = MeshFunction('size_t', mesh, 1, 0)
    _DfgCylinder().mark(markers, 1)
    dsc = Measure('ds', domain=mesh, subdomain_data=markers)(1)
    n = FacetNormal(mesh)
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
        if log is not None and steps % 100 == 0:
            log(steps, change)
    gu = grad(u0)

    def traction(a):
        return mu * ((gu[a, 0] + gu[0, a]) * n[0]
                     + (gu[a, 1] + gu[1, a]) * n[1]) - p0 * n[a]

    scale = 2.0 / (rho * DFG_UMEAN**2 * DFG_D)
    c_d = -scale * assemble(traction(0) * dsc)
    c_l = -scale * assemble(traction(1) * dsc)
    return c_d, c_l, steps, change, mesh


# h = 0.005 (72 facets on the cylinder).  Measured there: c_D = 5.56061
# (-0.34 %), c_L = 0.010674 (+0.5 %), the same to 7 digits for dt = 0.01 and
# 0.03 (the fixed point does not depend on dt); about 1200-2600 steps, a few
# seconds.  (At dt = 0.1 the momentum solve's GMRES stalls: its
# preconditioners are built for mass-dominated systems.)
DFG_MESH = (440, 82)
DFG_DT = 0.02


def test_dfg_2d1(hip):
    t0 = time.time()
    c_d, c_l, steps, change, mesh = dfg_coefficients(
        DFG_MESH[0], DFG_MESH[1], DFG_DT)
    print('DFG 2D-1 on %d cells: c_D = %.6f (%.3f %%), c_L = %.6f (%.1f %%), '
          '%d steps, change %.1e, %.1f s' % (
              mesh.num_cells(), c_d, 100 * (c_d / DFG_CD - 1), c_l,
              100 * (c_l / DFG_CL - 1), steps, change, time.time() - t0))
    assert change < 1.0e-10
    assert _rel(c_d, DFG_CD) < 0.01
    assert _rel(c_l, DFG_CL) < 0.20
