# -*- coding: utf-8 -*-
'''UFL-style forms (flow_amd/fem/forms.py) on the host: names, tensor
expansion, degree estimation, the register-program compiler and its limits,
the unchanged arithmetic of Constants, and the numpy evaluator of
tests/form_reference.py pinned by closed forms.  No GPU needed.'''
import os
import re
import sys

import numpy
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from flow_amd import fem, materials, message, _hip, device   # noqa: E402
from flow_amd.fem import (                                   # noqa: E402
    assemble, dx, SpatialCoordinate, as_vector, sqrt, exp, ln, sin, cos, dot,
    inner, grad, div, curl, begin, end, info, forms,
    )
import form_reference as fref                                # noqa: E402


def _spaces(mesh):
    return (fem.FunctionSpace(mesh, 'CG', 1), fem.FunctionSpace(mesh, 'CG', 2),
            fem.VectorFunctionSpace(mesh, 'CG', 2))


def test_names_and_no_cpu_fallback():
    assert begin is message.begin and end is message.end and info is message.info
    if device.on_gpu():
        pytest.skip('GPU present')
    mesh = fem.UnitSquareMesh(2, 2)
    with pytest.raises(_hip.HipError):
        assemble(1.0 * dx(mesh))
    P1 = fem.FunctionSpace(mesh, 'CG', 1)
    with pytest.raises(_hip.HipError):
        fem.project(sqrt(SpatialCoordinate(mesh)[0]), P1)


def test_tensor_expansion():
    mesh = fem.UnitSquareMesh(2, 2)
    _, _, W = _spaces(mesh)
    u = fem.Function(W)
    e = inner(grad(u), grad(u))
    assert e.shape == () and e.deg == 2
    terms = []

    def walk(n):
        if n[0] == 'add':
            walk(n[1])
            walk(n[2])
        else:
            terms.append(n)
    walk(e.comps)
    assert len(terms) == 4
    assert sorted((t[1][2], t[1][3]) for t in terms) == \
        [(0, 1), (0, 2), (1, 1), (1, 2)]
    assert all(t[0] == 'mul' and t[1] == t[2] and t[1][1] is u for t in terms)
    # div u = du0/dx + du1/dy, curl u = du1/dx - du0/dy
    assert div(u).comps == ('add', ('field', u, 0, 1), ('field', u, 1, 2))
    assert curl(u).comps == ('sub', ('field', u, 1, 1), ('field', u, 0, 2))
    assert grad(u).shape == (2, 2) and grad(u).deg == 1
    assert grad(u)[1, 0].comps == ('field', u, 1, 1)
    assert u.dx(1)[0].comps == ('field', u, 0, 2)
    x = SpatialCoordinate(mesh)
    assert dot(x, x).comps == ('add', ('mul', ('x', 0), ('x', 0)),
                               ('mul', ('x', 1), ('x', 1)))
    assert grad(x[0] * x[1]).comps == [('x', 1), ('x', 0)]


def test_degree_estimates():
    mesh = fem.UnitSquareMesh(2, 2)
    P1, P2, W = _spaces(mesh)
    p, th, u = fem.Function(P1), fem.Function(P2), fem.Function(W)
    x, y = SpatialCoordinate(mesh)[0], SpatialCoordinate(mesh)[1]
    e3 = fem.Expression('x[0]', degree=3)
    c = fem.Constant(2.0)
    table = [
        (p, 1), (th, 2), (e3, 3), (x, 1), (c * p, 1), (p + th, 2),
        (p * th, 3), (inner(u, u), 4), (dot(u, u), 4), (p / th, 3),
        (th**3, 6), (th**0.5, 4), (th**c, 4), (sqrt(th), 4), (exp(p), 3),
        (ln(th), 4), (sin(x), 3), (cos(th), 4), (abs(th), 2), (-th, 2),
        (grad(th)[0], 1), (div(u), 1), (curl(u), 1), (th.dx(0), 1),
        (grad(p)[0], 0), (as_vector([p, th])[0], 2), (2.0 * e3 * y, 4),
        (sqrt(u[0]**2 + u[1]**2), 6),
        ]
    for f, deg in table:
        assert forms.as_form(f).deg == deg, (f, deg)
    # the Boussinesq buoyancy: 12 for density(theta), 13 with y, 14 with P1
    rho = materials.density(th)
    assert rho.deg == 12
    f = rho * 9.81 * y
    assert f.deg == 13
    assert forms.projection_degree(f, 1) == 14
    assert forms.projection_degree(f, 1, {'quadrature_degree': 4}) == 4
    assert (th * dx).degree() == 2
    assert (th * dx(metadata={'quadrature_degree': 7})).degree() == 7
    assert (th * dx(mesh, metadata={'quadrature_degree': 3})).degree() == 3
    assert (1.0 * dx(domain=mesh)).degree() == 0
    prog = forms.Program([f.comps])
    assert len(prog.code) <= forms.MAX_PROGRAM
    with pytest.raises(ValueError, match='at most 30'):
        forms.check_degree(31)


def test_shape_errors():
    mesh = fem.UnitSquareMesh(2, 2)
    P1, P2, W = _spaces(mesh)
    u, p = fem.Function(W), fem.Function(P1)
    with pytest.raises(ValueError, match='scalar integrands'):
        assemble(u * dx)
    with pytest.raises(ValueError, match='rank 3'):
        grad(grad(u))
    with pytest.raises(ValueError):
        u + p
    with pytest.raises(ValueError):
        sqrt(u)
    with pytest.raises(ValueError, match='no mesh'):
        forms.form_mesh((fem.Constant(1.0) * dx).integrand)
    other = fem.UnitSquareMesh(3, 3)
    q = fem.Function(fem.FunctionSpace(other, 'CG', 1))
    with pytest.raises(ValueError, match='two different meshes'):
        p * q
    with pytest.raises(ValueError, match='two different meshes'):
        p * dx(other)


def test_compiler_limits_and_programs():
    mesh = fem.UnitSquareMesh(2, 2)
    P1, P2, W = _spaces(mesh)
    ops = forms.OPS
    # the opcodes are the header's
    header = open(os.path.join(ROOT, 'include', 'flow_hip.h')).read()
    for name, code in ops.items():
        m = re.search(r'#define FLOW_FORM_OP_%s (\d+)' % name.upper(), header)
        assert m and int(m.group(1)) == code, name
    for name in ('MAX_PROGRAM', 'REGISTERS', 'MAX_CONSTANTS', 'MAX_FIELDS',
                 'MAX_EXPRESSIONS'):
        m = re.search(r'#define FLOW_FORM_%s (\d+)' % name, header)
        assert int(m.group(1)) == getattr(forms, name) == \
            getattr(_hip, 'FORM_' + name)
    u = fem.Function(W)
    prog = forms.Program([sqrt(u[0]**2 + u[1]**2).comps])
    assert [c[0] for c in prog.code] == [ops[o] for o in (
        'field', 'mul', 'field', 'mul', 'add', 'sqrt', 'out')]
    assert prog.nregs == 2 and len(prog.fields) == 2
    # integer powers are multiplies (x^5: square, square, multiply)
    x = SpatialCoordinate(mesh)[0]
    prog = forms.Program([(x**5).comps])
    assert [c[0] for c in prog.code].count(ops['mul']) == 3
    assert ops['pow'] not in [c[0] for c in prog.code]
    assert ops['pow'] in [c[0] for c in forms.Program([(x**0.5).comps]).code]
    # too long
    e = x
    for i in range(40):
        e = e * (x + 1.0)
    with pytest.raises(ValueError, match='instructions: the limit is 64'):
        forms.Program([e.comps])
    # too many registers: a balanced tree of depth 4 needs 9
    def balanced(d):
        return x if d == 0 else balanced(d - 1) * balanced(d - 1) + \
            balanced(d - 1) * balanced(d - 1)
    with pytest.raises(ValueError, match='registers'):
        forms.Program([balanced(4).comps])
    # too many fields / constants
    fs = [fem.Function(P1) for _ in range(7)]
    with pytest.raises(ValueError, match='field components'):
        forms.Program([sum(fs[1:], fs[0]).comps])
    with pytest.raises(ValueError, match='constants'):
        forms.Program([sum((x + float(i) for i in range(40)), x).comps])


def test_old_arithmetic_unchanged():
    c = fem.Constant(2.0)
    assert isinstance(c * 3.0, fem.Constant) and (c * 3.0).values()[0] == 6.0
    assert isinstance(3.0 * c, fem.Constant)
    assert isinstance(c / 4.0, fem.Constant) and (c / 4.0).values()[0] == 0.5
    cv = fem.Constant((1.0, -2.0))
    assert numpy.allclose((cv * 2).values(), [2.0, -4.0])
    mesh = fem.UnitSquareMesh(2, 2)
    P1 = fem.FunctionSpace(mesh, 'CG', 1)
    p = fem.Function(P1)
    ne = fem.NodalExpression(lambda t: t, [p])
    out = ne * fem.Constant((0.0, -9.81))
    assert isinstance(out, fem.NodalExpression)
    assert numpy.allclose(out.scale, [0.0, -9.81])
    # identity hashing stays (no __eq__ / __hash__ defined)
    for obj in (c, p, fem.Expression('x[0]', degree=1)):
        assert type(obj).__eq__ is object.__eq__
        assert type(obj).__hash__ is object.__hash__
        assert {obj: 1}[obj] == 1
    assert isinstance(c * p, forms.FormExpr)
    assert isinstance(p * c, forms.FormExpr)
    assert isinstance(numpy.float64(2.0) * p, forms.FormExpr)


def test_host_evaluator_closed_forms():
    '''int x^a y^b over [x0, x1] x [y0, y1], the area, and a P2 interpolant of
    a quadratic against its exact integrals.'''
    x0, x1, y0, y1 = 0.5, 2.0, -1.0, 1.5
    mesh = fem.RectangleMesh(fem.Point(x0, y0), fem.Point(x1, y1), 5, 4)
    X = SpatialCoordinate(mesh)
    assert abs(fref.functional(1.0 * dx(mesh)) - mesh.cell_areas().sum()) \
        < 1e-14 * mesh.cell_areas().sum()
    for a, b in ((0, 0), (1, 0), (2, 3), (4, 1), (3, 5)):
        exact = (x1**(a + 1) - x0**(a + 1)) / (a + 1) * \
            (y1**(b + 1) - y0**(b + 1)) / (b + 1)
        got = fref.functional(X[0]**a * X[1]**b * dx)
        assert abs(got - exact) < 1e-13 * max(1.0, abs(exact)), (a, b)
    # P2 interpolant of (x^2 + x y, y^2 - 3 x): exact div and curl integrals
    W = fem.VectorFunctionSpace(mesh, 'CG', 2)
    u = fem.Function(W)
    xy = W.layout.dof_coords
    u.set_array(numpy.concatenate([xy[:, 0]**2 + xy[:, 0] * xy[:, 1],
                                   xy[:, 1]**2 - 3 * xy[:, 0]]))
    area = (x1 - x0) * (y1 - y0)
    # div u = 2x + y + 2y = 2x + 3y, curl u = -3 - x
    mx = 0.5 * (x0 + x1) * area
    my = 0.5 * (y0 + y1) * area
    assert abs(fref.functional(div(u) * dx) - (2 * mx + 3 * my)) < 1e-12
    assert abs(fref.functional(curl(u) * dx) - (-3 * area - mx)) < 1e-12
    # the load vector sums to the integral (partition of unity)
    P1 = fem.FunctionSpace(mesh, 'CG', 1)
    b = fref.load_vector(X[0] * X[1], P1)
    assert abs(b.sum() - fref.functional(X[0] * X[1] * dx)) < 1e-13
