# -*- coding: utf-8 -*-
'''
conditional, max_value / min_value / sign / tanh, the cell geometry operands
and the SUPG tau operand on the host (flow_amd/fem/forms.py): opcodes against
the header, degree estimation, spatial and Gateaux derivatives against central
differences of the numpy evaluator of tests/conditional_reference.py, the
distribution of conditionals over argument tables, every refusal that needs no
device, the register need of nested selects, and the numpy interpreter of the
instruction stream against the tree evaluator.  No GPU.
'''
import os
import re

import numpy
import pytest

from flow_amd import fem, stabilization
from flow_amd.fem import (
    TestFunction, TrialFunction, dx, ds, dot, inner, grad, derivative, forms,
    SpatialCoordinate, conditional, lt, le, gt, ge, eq, ne, And, Or, Not,
    max_value, min_value, sign, tanh, exp, sqrt, CellVolume, Circumradius,
    CellDiameter, as_vector,
    )

import conditional_reference as cref
import newton_reference as nref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _meshes():
    return [fem.UnitSquareMesh(12, 9),
            fem.karman_channel(60, 14, fitted=True),
            fem.karman_channel_graded(lcar=1.0e-2)]


def _spaces(n=3):
    mesh = fem.UnitSquareMesh(n, n)
    return (mesh, fem.FunctionSpace(mesh, 'CG', 1),
            fem.FunctionSpace(mesh, 'CG', 2))


def test_opcodes_are_the_headers():
    header = open(os.path.join(ROOT, 'include', 'flow_hip.h')).read()
    found = dict((name.lower(), int(code)) for name, code in re.findall(
        r'#define FLOW_FORM_OP_(\w+) (\d+)', header))
    assert found == forms.OPS
    # the old numbers did not move, the new ones follow them
    assert forms.OPS['normal'] == 18
    new = ('lt', 'le', 'eq', 'ne', 'select', 'min', 'max', 'sign', 'tanh',
           'cell')
    assert [forms.OPS[n] for n in new] == list(range(19, 29))


def test_degree_estimation():
    mesh, V1, V2 = _spaces()
    u1, u2 = fem.Function(V1), fem.Function(V2)
    x = SpatialCoordinate(mesh)
    # conditional: the larger branch; the condition does not count
    assert conditional(gt(u2**3, 0.0), u1, 1.0).deg == 1
    assert conditional(gt(u1, 0.0), u1, u2 * u2).deg == 4
    assert max_value(u1, u2).deg == 2 and min_value(u2 * u1, 1.0).deg == 3
    assert sign(u2).deg == 2
    assert tanh(u2).deg == 4 and tanh(x[0]).deg == 3
    for g in (CellVolume, Circumradius, CellDiameter):
        assert g(mesh).deg == 0 and g(mesh).mesh is mesh
        assert (g(mesh) * u2).deg == 2
    # tensors: component by component
    c = conditional(lt(x[0], 0.5), as_vector([u1, 1.0]), grad(u2))
    assert c.shape == (2,) and c.deg == 1
    assert c.comps[0][0] == 'cond' and c.comps[1][0] == 'cond'
    with pytest.raises(ValueError, match='shapes'):
        conditional(lt(x[0], 0.5), grad(u2), u1)
    # the tau operand: degree 1, an 'expr' leaf that carries its mesh
    W = fem.VectorFunctionSpace(mesh, 'CG', 2)
    tau = stabilization.supg(mesh, fem.Function(W), 0.1, 1)
    t = forms.as_form(tau)
    assert t.deg == 1 and t.mesh is mesh and t.comps == ('expr', tau, 0)
    assert (u1 * tau).deg == 2


def _switch(mesh, d=0):
    '''A condition that holds on about half of the mesh and does not depend
    on the state: x_d > its mean over the vertices.'''
    return gt(SpatialCoordinate(mesh)[d], float(mesh.points[:, d].mean()))


def _residuals(mesh, V, u):
    '''[(name, F)]: residuals with the new nodes whose switching surfaces do
    not depend on u, or stay a distance of order 1 from its range 1 <= u <= 2
    (so that the derivative exists and a perturbation of 1e-6 flips no
    point).'''
    v = TestFunction(V)
    W = fem.VectorFunctionSpace(mesh, 'CG', 2)
    b = fem.Function(W)
    xy = W.layout.dof_coords
    b.set_array(numpy.concatenate([1.0 + xy[:, 1], 0.5 - 0.3 * xy[:, 0]]))
    tau = stabilization.supg(mesh, b, 0.05, V.degree)
    h = CellDiameter(mesh)
    step = conditional(_switch(mesh), 10.0, 0.0)      # 10 or 0: u^2 is in [1, 4]
    return [
        ('conditional', conditional(_switch(mesh), u**2, exp(u)) * v * dx),
        ('conditional, nested',
         conditional(_switch(mesh), conditional(_switch(mesh, 1), u**3, u),
                     u.dx(0) * u) * v.dx(0) * dx),
        ('max_value', max_value(u**2, step) * v * dx),
        ('min_value', min_value(u**2, step) * u * v * dx),
        ('both taken at once', (max_value(u, 0.5) * min_value(u, 3.0)
                                + max_value(u, 2.5)) * u * v * dx),
        ('sign', sign(SpatialCoordinate(mesh)[1]
                      - float(mesh.points[:, 1].mean())) * u**2 * v * dx),
        ('tanh', (tanh(u) * v + tanh(0.2 * u) * u.dx(0) * v) * dx),
        ('geometry', (h * u**2 * inner(grad(u), grad(v))
                      + u**3 / CellVolume(mesh) * Circumradius(mesh)**2 * v)
         * dx),
        ('tau', tau * u**2 * dot(b, grad(v)) * dx),
        ]


def test_gateaux_derivative_against_central_differences():
    '''The method and e of tests/test_nonlinear_forms_host.py: J(u) w of J =
    derivative(F, u) against central differences of the evaluator on the
    unextracted trees, e = 1e-6 |u|_inf, max-norm relative to |J w|_inf,
    bound 7e-6.'''
    worst = {}
    for m, mesh in enumerate(_meshes()):
        for k in (1, 2):
            V = fem.FunctionSpace(mesh, 'CG', k)
            u = nref.state(V)
            w = numpy.random.RandomState(5).uniform(-1.0, 1.0, V.N)
            eps = 1.0e-6 * numpy.abs(u.array()).max()
            for name, F in _residuals(mesh, V, u):
                J = derivative(F, u)
                assert J.rank == 2
                Jw = cref.matrix(J).dot(w)
                fd = cref.central_difference(F, u, w, eps)
                e = numpy.abs(Jw - fd).max() / numpy.abs(Jw).max()
                print('mesh %d P%d %-22s %.2e' % (m, k, name, e))
                worst[name] = max(worst.get(name, 0.0), e)
    print(worst)
    assert len(worst) == 9
    assert max(worst.values()) < 7.0e-6


def test_gateaux_rules():
    mesh, V1, V2 = _spaces()
    u = fem.Function(V2)
    v = TestFunction(V2)
    U = ('field', u, 0, 0)
    A = ('arg', 1, 0, V2)
    c = ('gt', ('x', 0), ('num', 0.5))
    # the condition is kept, never differentiated
    t = forms.s_gateaux(('cond', ('gt', U, ('num', 0.0)), U, ('neg', U)), u,
                        1, V2)
    assert t == ('cond', ('gt', U, ('num', 0.0)), A, ('neg', A))
    # max_value(a, b) -> conditional(gt(a, b), a', b'), min_value likewise
    assert forms.s_gateaux(('max', U, ('x', 0)), u, 1, V2) == \
        ('cond', ('gt', U, ('x', 0)), A, forms.ZERO)
    assert forms.s_gateaux(('min', U, ('x', 0)), u, 1, V2) == \
        ('cond', ('lt', U, ('x', 0)), A, forms.ZERO)
    # sign: 0; tanh' = 1 - tanh^2; geometry, tau: 0; equal branches fold
    assert forms.s_gateaux(('sign', U), u, 1, V2) == forms.ZERO
    assert forms.s_gateaux(('tanh', U), u, 1, V2) == \
        ('mul', ('sub', forms.ONE, ('powi', ('tanh', U), 2)), A)
    assert forms.s_gateaux(('cell', mesh, 2), u, 1, V2) == forms.ZERO
    assert forms.s_gateaux(('cond', c, ('x', 1), ('x', 0)), u, 1, V2) \
        == forms.ZERO
    # tau is a coefficient: derivative zero with respect to ANY Function,
    # the convection field included
    W = fem.VectorFunctionSpace(mesh, 'CG', 2)
    b = fem.Function(W)
    tau = stabilization.supg(mesh, b, 0.1, 2)
    F = tau * u * dot(b, grad(v)) * dx
    J = derivative(F, u)
    rank, tab = J.argument_table()
    assert rank == 2 and tab[1][0] is not None and tab[0][0] is None
    G = tau * v * dx
    with pytest.raises(ValueError, match='does not depend on u'):
        derivative(G, u)


def test_spatial_derivative_against_central_differences():
    '''f.dx(d) of expressions of every new node at points inside the cells
    against (f(x + e) - f(x - e)) / 2e of the same evaluator, e = 1e-6 of the
    cell's diameter (both points stay in the cell, where f is smooth: the
    conditions switch on cell-wise constant or far-away data).  Error:
    O(e^2) + O(eps / e), the bound that of the Gateaux test, 7e-6.'''
    mesh = fem.UnitSquareMesh(6, 5)
    V2 = fem.FunctionSpace(mesh, 'CG', 2)
    u = nref.state(V2)
    h = CellDiameter(mesh)
    X = SpatialCoordinate(mesh)
    big = gt(CellVolume(mesh), float(numpy.median(
        cref.cell_quantities(mesh)[:, 0])) * (1 + 1e-9))
    odd = gt(Circumradius(mesh) * (1.0 + X[0] * 0.0), 0.0)
    exprs = [
        ('conditional', conditional(big, u**2 * X[0], exp(u) + X[1])),
        ('conditional, And/Or/Not',
         conditional(Or(And(big, odd), Not(odd)), tanh(u), u**3)),
        ('max_value', max_value(u**2, 0.5) + max_value(u, 2.5 + X[0])),
        ('min_value', min_value(u**2, 0.5 + X[1]) * u + min_value(u, 9.0)),
        ('sign', sign(u - 0.25) * u**2 + sign(X[0] - 7.0) * u),
        ('tanh', tanh(u * X[0]) / (1 + tanh(0.1 * u)**2)),
        ('geometry', h * u**2 + u / CellVolume(mesh) * Circumradius(mesh)),
        ]
    nc = mesh.num_cells()
    cells = numpy.arange(nc)
    P = mesh.points[mesh.cell_vertices]
    lam = numpy.array([0.3, 0.45, 0.25])
    pts = numpy.einsum('v,cvd->cd', lam, P)
    e = 1.0e-6 * cref.cell_quantities(mesh)[:, 2]
    worst = {}
    for name, f in exprs:
        for d in (0, 1):
            step = numpy.zeros((nc, 2))
            step[:, d] = e
            exact = cref.point_values(f.dx(d), mesh, pts, cells)[0]
            fd = (cref.point_values(f, mesh, pts + step, cells)[0]
                  - cref.point_values(f, mesh, pts - step, cells)[0]) / (2 * e)
            err = numpy.abs(exact - fd).max() / numpy.abs(exact).max()
            print('%-26s d/dx%d %.2e' % (name, d, err))
            worst[name] = max(worst.get(name, 0.0), err)
    assert len(worst) == 7 and max(worst.values()) < 7.0e-6
    # the rules themselves
    U = ('field', u, 0, 0)
    assert forms.s_diff(('cell', mesh, 0), 0) == forms.ZERO
    assert forms.s_diff(('sign', U), 1) == forms.ZERO
    assert forms.s_diff(('max', U, ('x', 0)), 0) == \
        ('cond', ('gt', U, ('x', 0)), ('field', u, 0, 1), forms.ONE)
    assert forms.s_diff(('tanh', U), 1) == \
        ('mul', ('sub', forms.ONE, ('powi', ('tanh', U), 2)),
         ('field', u, 0, 2))


def test_conditionals_distribute_over_argument_tables():
    mesh, V1, V2 = _spaces()
    u, v = TrialFunction(V2), TestFunction(V2)
    f = fem.Function(V2)
    c = _switch(mesh)
    F = ('field', f, 0, 0)
    # the argument in one branch only: zero where the branch lacks the term
    rank, tab = (conditional(c, f * v, 0.0) * dx).argument_table()
    assert rank == 1 and tab[1] is None and tab[2] is None
    assert tab[0] == ('cond', c.tree, F, forms.ZERO)
    rank, tab = (conditional(c, v, f * v.dx(0)) * dx).argument_table()
    assert rank == 1 and tab[2] is None
    assert tab[0] == ('cond', c.tree, forms.ONE, forms.ZERO)
    assert tab[1] == ('cond', c.tree, forms.ZERO, F)
    # in both branches: one conditional per term
    rank, tab = (conditional(c, f * u * v, inner(grad(u), grad(v))) * dx
                 ).argument_table()
    assert rank == 2
    assert tab[0][0] == ('cond', c.tree, F, forms.ZERO)
    assert tab[1][1] == tab[2][2] == ('cond', c.tree, forms.ZERO, forms.ONE)
    assert sum(t is not None for row in tab for t in row) == 3
    # equal coefficients in the two branches need no conditional
    rank, tab = (conditional(c, u * v, u * v + u.dx(0) * v) * dx
                 ).argument_table()
    assert tab[0][0] == forms.ONE
    assert tab[0][1] == ('cond', c.tree, forms.ZERO, forms.ONE)
    # nested, and under a product with the other argument
    c2 = _switch(mesh, 1)
    inner_c = conditional(c2, f * u, u.dx(1))
    rank, tab = (conditional(c, inner_c, 3.0 * u) * v * dx).argument_table()
    assert rank == 2
    assert tab[0][0] == ('cond', c.tree, ('cond', c2.tree, F, forms.ZERO),
                         ('num', 3.0))
    assert tab[0][2] == ('cond', c.tree,
                         ('cond', c2.tree, forms.ZERO, forms.ONE), forms.ZERO)
    # the tables reproduce the unextracted tree: the host matrix of the form
    # (basis functions substituted into the tree) against the matrix built
    # from its table
    form = conditional(c, inner_c, 3.0 * u) * v * dx
    A = cref.matrix(form).toarray()
    B = numpy.zeros_like(A)
    for b in range(3):
        for a in range(3):
            if tab[b][a] is None:
                continue
            ua = u if a == 0 else u.dx(a - 1)
            vb = v if b == 0 else v.dx(b - 1)
            coef = forms.FormExpr(tab[b][a], (), 2, mesh)
            B += cref.matrix(coef * ua * vb * dx(degree=form.degree())
                             ).toarray()
    assert numpy.abs(A - B).max() <= 1e-14 * numpy.abs(A).max()
    # derivative() puts its argument into the branches and the result passes
    g = fem.Function(V2)
    R = conditional(gt(g, 0.5), g**2, max_value(g, 0.1)) * v * dx
    rank, tab = derivative(R, g).argument_table()
    assert rank == 2 and tab[0][0][0] == 'cond'
    # compiled like any other table, and shared between J and F
    prog = forms.argument_program(tab, 2)
    assert forms.OPS['select'] in [ins[0] for ins in prog.code]
    tF = R.argument_table()[1]
    both = forms.newton_program(tab, tF)
    assert both.nout == 12 and both.slots == [0, 9]


def test_refusals():
    mesh, V1, V2 = _spaces()
    u, v = TrialFunction(V2), TestFunction(V2)
    f = fem.Function(V2)
    c = gt(f, 0.5)
    # a condition is not a number
    for bad in (lambda: c + 1.0, lambda: 2.0 * c, lambda: c * f, lambda: f * c,
                lambda: c / 2.0, lambda: -c, lambda: c**2, lambda: abs(c),
                lambda: c * dx, lambda: tanh(c), lambda: max_value(c, 0.0),
                lambda: conditional(c, c, 1.0), lambda: as_vector([c, 1.0]),
                lambda: fem.sqrt(c)):
        with pytest.raises((TypeError, ValueError),
                           match='condition .* is not a scalar operand'):
            bad()
    with pytest.raises(TypeError, match='no truth value'):
        bool(c)
    # ... and a number is not a condition
    for bad in (lambda: conditional(f, 1.0, 2.0), lambda: And(c, f),
                lambda: Or(1.0, c), lambda: Not(f),
                lambda: conditional(True, 1.0, 2.0)):
        with pytest.raises(TypeError, match='a condition is expected'):
            bad()
    with pytest.raises(ValueError, match='conditions compare scalars'):
        gt(grad(f), 0.0)
    # arguments: in a condition, under max_value / min_value / sign / tanh
    cases = [
        (conditional(gt(v, 0.0), f, 1.0) * v * dx, 'condition of a conditional'),
        (conditional(gt(f * u, 0.0), u, 2.0 * u) * v * dx,
         'condition of a conditional'),
        (max_value(v, 0.0) * dx, 'max_value'),
        (min_value(f, u) * v * dx, 'min_value'),
        (sign(v) * f * dx, 'sign'),
        (tanh(u) * v * dx, 'tanh'),
        ]
    for form, name in cases:
        with pytest.raises(ValueError, match='not linear.*%s' % name):
            form.argument_table()
    # the pinned refusal of arguments under ds holds inside a conditional
    with pytest.raises(NotImplementedError, match='under ds'):
        conditional(c, v, 0.0) * ds
    # a geometry operand of another mesh
    other = fem.UnitSquareMesh(2, 2)
    for g in (CellVolume, Circumradius, CellDiameter):
        with pytest.raises(ValueError, match='two different meshes'):
            g(other) * f
        with pytest.raises(ValueError, match='two different meshes'):
            g(other) * dx(mesh)
        with pytest.raises(ValueError, match='two different meshes'):
            conditional(gt(g(other), 1.0), f, 0.0)
        with pytest.raises(TypeError, match='takes a mesh'):
            g(V2)
    # tau: a scalar on its mesh; not at points (an Expression-like leaf)
    W = fem.VectorFunctionSpace(mesh, 'CG', 2)
    tau = stabilization.supg(mesh, fem.Function(W), 0.1, 1)
    with pytest.raises(ValueError, match='two different meshes'):
        tau * fem.Function(fem.FunctionSpace(other, 'CG', 1))
    with pytest.raises(ValueError, match='cannot be evaluated at points'):
        forms.point_program(tau * f)
    # no spatial derivatives of tau, and the message names it
    for bad in (lambda: grad(tau * f), lambda: forms.as_form(tau).dx(0),
                lambda: fem.div(tau * grad(f))):
        with pytest.raises(NotImplementedError, match='SUPG tau'):
            bad()
    # the limits of flow_form raise a ValueError of their own kind
    assert issubclass(forms.ProgramLimit, ValueError)
    big = ('field', f, 0, 0)
    for i in range(70):
        big = ('add', big, ('x', i % 2))
    with pytest.raises(forms.ProgramLimit, match='instructions'):
        forms.Program([big])
    # the normal stays a ds-only operand inside a conditional
    n = fem.FacetNormal(mesh)
    with pytest.raises(ValueError, match='FacetNormal'):
        conditional(c, n[0], 0.0) * dx


def test_register_need_of_nested_selects():
    mesh, V1, V2 = _spaces()
    f = fem.Function(V2)
    F = ('field', f, 0, 0)
    need = forms.Program.need
    c = ('lt', F, ('num', 0.0))
    # three live values: else-value, condition (2 registers), then-value
    assert need(('cond', c, F, ('x', 0))) == 3
    prog = forms.Program([('cond', c, F, ('x', 0))])
    assert prog.nregs == 3
    names = {v: k for k, v in forms.OPS.items()}
    # the largest need first: the condition; the else-value is then moved
    assert [names[i[0]] for i in prog.code] == [
        'field', 'const', 'lt', 'coord', 'field', 'select', 'mov', 'out']
    assert forms._count(('cond', c, F, ('x', 0))) == 7
    # else-value first where nothing needs more: no mov
    prog = forms.Program([('cond', ('reg', 7), F, ('x', 0))])
    assert [names[i[0]] for i in prog.code] == [
        'coord', 'mov', 'field', 'select', 'out']
    assert prog.code[3] == (forms.OPS['select'], 0, 1, 2)
    # gt / ge are lt / le with the operands swapped
    prog = forms.Program([('ge', ('x', 0), ('x', 1))])
    o = forms.OPS
    assert prog.code[:3] == [(o['coord'], 0, 1, 0), (o['coord'], 1, 0, 0),
                             (o['le'], 0, 0, 1)]
    assert 'gt' not in o and 'ge' not in o
    # nesting in the then-value costs two registers a level: depth 3 fits
    # (need 7), depth 4 needs 9 > 8 registers
    def nest(depth):
        t = F
        for i in range(depth):
            t = ('cond', ('lt', ('x', 0), ('num', float(i))), t, ('x', 1))
        return t

    def deep(depth):
        # every level holds its else-value and its condition while the
        # then-value, the deepest tree, is computed
        t = ('add', F, ('x', 0))
        for i in range(depth):
            t = ('cond', ('lt', ('add', ('x', 0), ('x', 1)), ('num', float(i))),
                 ('mul', t, t), ('add', t, ('x', 1)))
        return t

    assert need(nest(6)) == 3          # a chain in the else-direction is flat
    forms.Program([nest(6)])
    needs = [need(deep(d)) for d in range(1, 9)]
    print('register need of nested selects:', needs)
    assert needs == sorted(needs) and needs[0] >= 3
    fits = [d for d in range(1, 9) if need(deep(d)) <= forms.REGISTERS]
    over = [d for d in range(1, 9) if need(deep(d)) > forms.REGISTERS]
    assert fits and over
    forms.Program([deep(1)])
    with pytest.raises(ValueError, match='more than 8 registers'):
        forms.Program([deep(over[0])])


def test_program_interpreter_agrees_bit_for_bit():
    '''The numpy interpreter of the instruction stream (the register machine
    with the opcodes from 19 up) against the tree evaluator's operations on
    the same leaf values: equal bits, for single programs, coefficient tables
    and the shared Newton program.  Leaves are uniform in [0.5, 2]: both
    sides of every condition occur.'''
    mesh, V1, V2 = _spaces()
    u = fem.Function(V2)
    g = fem.Function(V1)
    v = TestFunction(V2)
    X = SpatialCoordinate(mesh)
    h = CellDiameter(mesh)
    W = fem.VectorFunctionSpace(mesh, 'CG', 2)
    b = fem.Function(W)
    tau = stabilization.supg(mesh, b, 0.1, 2)
    Pe = sqrt(dot(b, b)) * h / (2 * 0.01)
    exprs = [
        conditional(gt(u, g), tanh(u) / h, max_value(u, 1.0) * X[0]),
        conditional(And(le(u, 1.2), Not(eq(g, X[1]))), min_value(u, g),
                    sign(u - 1.0) * Circumradius(mesh)),
        conditional(Or(lt(u, 0.8), ne(g, g)), CellVolume(mesh), u**2 - tau),
        conditional(ge(Pe, 100.0), (1 / tanh(Pe) - 1 / Pe) / Pe,
                    1.0 / 3 - Pe**2 / 45),
        conditional(gt(u, 1.0), conditional(lt(g, 1.0), u, g * u),
                    conditional(lt(g, 1.5), tanh(g), -u)),
        ]
    leaves = nref.Leaves(64, seed=2)
    for e in exprs:
        prog = forms.compile_trees([e.comps])
        got = cref.run_program(prog, leaves)
        want = cref.eval_tree(e.comps, leaves)
        assert numpy.isfinite(want).all()
        assert numpy.array_equal(got[0], want)
    # both branches were taken somewhere
    c = cref.eval_tree(('gt', exprs[0].comps[1][1], exprs[0].comps[1][2]),
                       leaves)
    assert 0 < c.sum() < len(c)
    # a residual, its Jacobian and the shared program of the two
    F = conditional(gt(u, g), tanh(u), max_value(u, 1.0)) * v * dx \
        + conditional(lt(g, 1.0), u, g * u) * u.dx(0) * v * dx
    for part in [p for _, p in F.terms()]:
        tF = part.argument_table()[1]
        tJ = derivative(part, u).argument_table()[1]
        want = {3 * bb + a: cref.eval_tree(tJ[bb][a], leaves)
                for bb in range(3) for a in range(3) if tJ[bb][a] is not None}
        want.update({9 + bb: cref.eval_tree(tF[bb], leaves)
                     for bb in range(3) if tF[bb] is not None})
        for share in (False, True):
            prog = forms.newton_program(tJ, tF, share=share)
            got = cref.run_program(prog, leaves)
            assert sorted(got) == sorted(want)
            for k in want:
                assert numpy.array_equal(got[k], want[k]), (share, k)
    # an untaken singular branch: 0/0 and inf - inf do not reach the result
    zero = nref.Leaves(8, seed=0)
    zero.values[('field', id(u), 0, 0)] = numpy.zeros(8)
    Pu = forms.as_form(u)
    xi = conditional(gt(Pu, 1e-5), (1 / tanh(Pu) - 1 / Pu) / Pu,
                     1.0 / 3 - Pu**2 / 45)
    got = cref.run_program(forms.Program([xi.comps]), zero)[0]
    assert numpy.array_equal(got, numpy.full(8, 1.0 / 3))


def test_existing_programs_are_unchanged():
    # the streams the other host tests pin hold no opcode from 19 up
    mesh, V1, V2 = _spaces()
    u = nref.state(V2)
    for name, F in nref.residuals(mesh, V2, u):
        for _, part in F.terms():
            rank, tab = part.argument_table()
            for prog in forms.argument_programs(tab, rank):
                assert max(ins[0] for ins in prog.code) <= forms.OPS['normal']


def test_lhs_rhs_split_an_integrand_of_both_ranks():
    '''The reference's SUPG term, R2 * tau * dot(conv, grad(v)) * dx with R2
    = -dot(conv, grad(u)) + source / rho_cp, is ONE integrand with a bilinear
    and a linear term: lhs / rhs split it by linearity, as UFL does; against
    the two terms written as separate forms (host evaluator, 1e-14).'''
    mesh = fem.UnitSquareMesh(4, 3)
    W = fem.VectorFunctionSpace(mesh, 'CG', 2)
    conv = fem.Function(W)
    xy = W.layout.dof_coords
    conv.set_array(numpy.concatenate([1.0 + xy[:, 1], 0.5 - 0.3 * xy[:, 0]]))
    source = fem.Expression('1.0 + x[0]*x[1]', degree=2)
    for k in (1, 2):
        V = fem.FunctionSpace(mesh, 'CG', k)
        u, v = TrialFunction(V), TestFunction(V)
        tau = stabilization.supg(mesh, conv, 0.05, k)
        R2 = - dot(conv, grad(u)) + source / 2.73
        f = u * v * dx + R2 * tau * dot(conv, grad(v)) * dx - source * v * dx
        a, L = fem.lhs(f), fem.rhs(f)
        assert [p.rank for _, p in a.terms()] == [2, 2]
        assert [(s, p.rank) for s, p in L.terms()] == [(-1.0, 1), (1.0, 1)]
        a2 = u * v * dx - dot(conv, grad(u)) * tau * dot(conv, grad(v)) * dx
        L2 = source * v * dx - source / 2.73 * tau * dot(conv, grad(v)) * dx
        A, A2 = cref.matrix(a), cref.matrix(a2)
        assert abs(A - A2).max() <= 1e-14 * abs(A2).max()
        b, b2 = cref.vector(L), cref.vector(L2)
        assert numpy.abs(b - b2).max() <= 1e-14 * numpy.abs(b2).max()
        # unsplit, the integrand has no one rank
        with pytest.raises(ValueError, match='differ in rank'):
            (R2 * tau * dot(conv, grad(v)) * dx).rank
