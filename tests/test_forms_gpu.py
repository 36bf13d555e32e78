# -*- coding: utf-8 -*-
'''
assemble / project of UFL-style integrands on the HIP path
(flow_amd/fem/forms.py, csrc/form_kernels.hip): exact integrals, the host
evaluator of tests/form_reference.py at the same rules, the forms the
reference's drivers write around a step, determinism, and an IPCS order test
whose pressure is shifted with assemble(sol_p*dx(mesh)).  Meshes stay small.
'''
import numpy
import pytest

from flow_amd import fem, materials
import flow_amd.navier_stokes as navsto
from flow_amd.fem import (
    assemble, dx, SpatialCoordinate, as_vector, sqrt, exp, ln, sin, cos, dot,
    inner, grad, div, curl,
    )

import form_reference as fref
import mms

pytestmark = pytest.mark.gpu


def _rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


def _meshes():
    return [fem.UnitSquareMesh(12, 9),
            fem.karman_channel(60, 14, fitted=True),
            fem.karman_channel_graded(lcar=1.0e-2)]


def _p2_field(W, funcs):
    u = fem.Function(W)
    xy = W.layout.dof_coords
    u.set_array(numpy.concatenate([f(xy[:, 0], xy[:, 1]) for f in funcs]))
    return u


def _host_projection(expr, V, fcp=None):
    import scipy.sparse.linalg as spla
    b = fref.load_vector(expr, V, fcp).reshape(V.dim, V.N)
    M = fem.assemble_mass(fem.FunctionSpace(V.mesh(), 'CG', V.degree)) \
        .to_scipy().tocsc()
    lu = spla.splu(M)
    return numpy.concatenate([lu.solve(b[a]) for a in range(V.dim)])


def test_area(hip):
    for mesh in _meshes():
        area = mesh.cell_areas().sum()
        assert _rel(assemble(1.0 * dx(mesh)), area) < 1e-14
        assert _rel(assemble(fem.Constant(1.0) * dx(domain=mesh)), area) < 1e-14


def test_exact_integrals(hip):
    x0, x1, y0, y1 = 0.5, 2.0, -1.0, 1.5
    mesh = fem.RectangleMesh(fem.Point(x0, y0), fem.Point(x1, y1), 9, 7)
    X = SpatialCoordinate(mesh)
    for a, b in ((0, 0), (1, 0), (2, 3), (4, 1), (3, 5), (7, 2)):
        exact = (x1**(a + 1) - x0**(a + 1)) / (a + 1) * \
            (y1**(b + 1) - y0**(b + 1)) / (b + 1)
        assert _rel(assemble(X[0]**a * X[1]**b * dx), exact) < 1e-13, (a, b)
    W = fem.VectorFunctionSpace(mesh, 'CG', 2)
    u = _p2_field(W, [lambda x, y: x**2 + x * y, lambda x, y: y**2 - 3 * x])
    area = (x1 - x0) * (y1 - y0)
    mx, my = 0.5 * (x0 + x1) * area, 0.5 * (y0 + y1) * area
    assert _rel(assemble(div(u) * dx), 2 * mx + 3 * my) < 1e-12
    assert _rel(assemble(curl(u) * dx), -3 * area - mx) < 1e-12
    # int u0 = int x^2 + x y
    ex = (x1**3 - x0**3) / 3 * (y1 - y0) + mx * 0.5 * (y0 + y1)
    assert _rel(assemble(u[0] * dx), ex) < 1e-12
    P1 = fem.FunctionSpace(mesh, 'CG', 1)
    p = fem.project(fem.Expression('sin(x[0])*x[1]', degree=3), P1)
    assert _rel(assemble(p * dx), fem.integral(p)) < 1e-12
    assert _rel(assemble(inner(u, u) * dx), fem.norm(u)**2) < 1e-12


def test_against_host_evaluator(hip):
    mesh = fem.karman_channel(60, 14, fitted=True)
    P1 = fem.FunctionSpace(mesh, 'CG', 1)
    P2 = fem.FunctionSpace(mesh, 'CG', 2)
    W = fem.VectorFunctionSpace(mesh, 'CG', 2)
    u = _p2_field(W, [lambda x, y: numpy.sin(20 * x) * y + 1.0,
                      lambda x, y: numpy.cos(30 * y) * x])
    p = fem.interpolate(fem.Expression('exp(x[0])*x[1] + 2', degree=3), P1)
    th = fem.interpolate(fem.Expression('0.5 + x[0]*x[1]', degree=2), P2)
    X = SpatialCoordinate(mesh)
    ex = fem.Expression('sin(40*x[0]) + x[1]', degree=4)
    ev = fem.Expression(('x[1]', 'x[0]*x[0]'), degree=2)
    c = fem.Constant(1.7)
    integrands = [
        inner(u, u), sqrt(u[0]**2 + u[1]**2), abs(u[0] - u[1]),
        curl(u)**2, inner(grad(u), grad(u)), div(u) * p, p**2.5,
        exp(th) * ln(p), sin(X[0] * 30) * cos(th), c * th**c / p,
        ex * u[0] + dot(ev, u), dot(grad(p), grad(th)), (p + 1.0)**-2,
        as_vector([X[1], -X[0]])[0] * th, 0.5 * inner(u, u) + p * th,
        ]
    for f in integrands:
        a = assemble(f * dx)
        assert _rel(a, fref.functional(f * dx)) < 1e-12, f
        b = fem.ops.form_load_vector(f, P2).cpu().numpy()
        ref = fref.load_vector(f, P2)
        assert numpy.abs(b - ref).max() < 1e-12 * numpy.abs(ref).max(), f
    a = assemble(th * u[0] * dx(metadata={'quadrature_degree': 2}))
    assert _rel(a, fref.functional(th * u[0] * dx(
        metadata={'quadrature_degree': 2}))) < 1e-12
    # vector-valued projection, and the projection solve
    f = as_vector([u[1] * p, sqrt(th)])
    got = fem.project(f, W).array()
    ref = _host_projection(f, W)
    assert numpy.abs(got - ref).max() < 1e-10 * numpy.abs(ref).max()


def test_driver_forms(hip):
    mesh = fem.karman_channel(60, 14, fitted=True)
    W = fem.VectorFunctionSpace(mesh, 'CG', 2)
    Q = fem.FunctionSpace(mesh, 'CG', 2)
    u1 = _p2_field(W, [lambda x, y: numpy.sin(20 * x) * y + 1.0,
                       lambda x, y: numpy.cos(30 * y) * x - 0.1])
    u0 = _p2_field(W, [lambda x, y: x * y, lambda x, y: numpy.sin(x + y)])
    # Karman step-size control: the magnitude at quadrature degree 4
    ux, uy = u1.split()
    fcp = {'quadrature_degree': 4}
    mag = sqrt(ux**2 + uy**2)
    got = fem.project(mag, Q, form_compiler_parameters=fcp).array()
    ref = _host_projection(mag, Q, fcp)
    assert numpy.abs(got - ref).max() < 1e-10 * numpy.abs(ref).max()
    # ... and the specialised kernel (its own 7-point rule, the same load
    # vector up to quadrature error of the non-polynomial |u|: loose)
    old = fem.project_magnitude(u1).array()
    assert numpy.abs(got - old).max() < 2e-2 * numpy.abs(old).max()
    # Boussinesq: the change of the velocity between two steps
    u1x, u1y = u1.split()
    u0x, u0y = u0.split()
    f = abs(u1x - u0x) + abs(u1y - u0y)
    got = fem.project(f, Q).array()
    ref = _host_projection(f, Q)
    assert numpy.abs(got - ref).max() < 1e-10 * numpy.abs(ref).max()
    # Boussinesq / sealed box: hydrostatic pressure of a uniform temperature
    P1 = fem.FunctionSpace(mesh, 'CG', 1)
    theta = fem.Function(fem.FunctionSpace(mesh, 'CG', 2))
    theta.assign(fem.Constant(293.0))
    g = -9.81
    y = SpatialCoordinate(mesh)[1]
    p = fem.project(materials.density(theta) * g * y, P1)
    want = materials.density(293.0) * g * P1.layout.dof_coords[:, 1]
    assert numpy.abs(p.array() - want).max() < 1e-12 * numpy.abs(want).max()


def test_determinism(hip):
    mesh = fem.karman_channel_graded(lcar=1.0e-2)
    W = fem.VectorFunctionSpace(mesh, 'CG', 2)
    u = _p2_field(W, [lambda x, y: numpy.sin(20 * x) * y,
                      lambda x, y: numpy.cos(30 * y) * x])
    f = sqrt(inner(u, u)) * dx
    vals = [assemble(f) for _ in range(3)]
    assert vals[0].hex() == vals[1].hex() == vals[2].hex()
    # a time loop re-assigns Constants and fields: no new upload, new values
    c = fem.Constant(1.0)
    a1 = assemble(c * u[0] * dx)
    c.assign(3.0)
    assert _rel(assemble(c * u[0] * dx), 3.0 * a1) < 1e-14


def test_ipcs_order_with_assembled_pressure_shift(hip):
    '''IPCS on the manufactured solution of tests/test_reference_counterparts
    (test_ipcs: same problem, meshes and steps), the pressure shifted as the
    reference's driver shifts it: by (assemble(sol_p*dx(mesh)) -
    assemble(p1*dx(mesh))) / assemble(1.0*dx(mesh)), with the exact pressure
    integrated through its lattice instead of its P1 projection.'''
    problem = mms.guermond2()
    method = navsto.IPCS(time_step_method='backward euler')
    mesh_sizes, Dt = [8, 16, 32], [1.0, 0.5]
    errors = {'u': numpy.empty((3, 2)), 'p': numpy.empty((3, 2))}
    (x0, y0), (x1, y1) = problem.domain
    for k, n in enumerate(mesh_sizes):
        mesh = fem.RectangleMesh(fem.Point(x0, y0), fem.Point(x1, y1), n, n,
                                 problem.diagonal)
        W = fem.VectorFunctionSpace(mesh, 'CG', 2)
        P = fem.FunctionSpace(mesh, 'CG', 1)
        mesh_area = assemble(1.0 * dx(mesh))
        for j, dt in enumerate(Dt):
            sol_u = fem.Expression(lambda x, t: problem.u(x, t),
                                   degree=problem.u_degree, t=0.0)
            sol_p = fem.Expression(lambda x, t: problem.p(x, t),
                                   degree=problem.p_degree, t=0.0)
            rhs0 = fem.Expression(lambda x, t: problem.f(x, t),
                                  degree=problem.f_degree, t=0.0)
            rhs1 = fem.Expression(lambda x, t: problem.f(x, t),
                                  degree=problem.f_degree, t=dt)
            sol_u.t = -dt
            u_1 = fem.project(sol_u, W)
            sol_u.t = 0.0
            u0 = fem.project(sol_u, W)
            p0 = fem.project(sol_p, P)
            sol_u.t = dt
            u1, p1 = method.step(
                fem.Constant(dt), {-1: u_1, 0: u0}, p0,
                u_bcs=[fem.DirichletBC(W, sol_u, 'on_boundary')], p_bcs=[],
                rho=fem.Constant(problem.rho), mu=fem.Constant(problem.mu),
                f={0: rhs0, 1: rhs1}, verbose=False, tol=1.0e-10)
            sol_p.t = dt
            errors['u'][k][j] = fem.errornorm(sol_u, u1)
            alpha = (assemble(sol_p * dx(mesh)) - assemble(p1 * dx(mesh))) \
                / mesh_area
            p1.vector()[:] += alpha
            errors['p'][k][j] = fem.errornorm(sol_p, p1)
    orders = {key: numpy.log(v[:, 0] / v[:, 1]) / numpy.log(Dt[0] / Dt[1])
              for key, v in errors.items()}
    assert (orders['u'] > method.order['velocity'] - 0.1).all(), orders
    assert (orders['p'] > method.order['pressure'] - 0.1).all(), orders
