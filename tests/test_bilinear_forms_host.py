# -*- coding: utf-8 -*-
'''
Forms of test and trial functions on the host (flow_amd/fem/forms.py): the
linearity extraction against hand-written tables, estimated degrees, the
vertex rule, lhs / rhs / Equation, every refusal that needs no device, and the
numpy evaluator of tests/bilinear_reference.py against closed forms.  No GPU.
'''
import numpy
import pytest

from flow_amd import fem
from flow_amd.fem import (
    TestFunction, TrialFunction, dx, ds, dot, inner, grad, as_vector, sin,
    sqrt, lhs, rhs, system, forms,
    )

import bilinear_reference as bref


def _spaces(n=3):
    mesh = fem.UnitSquareMesh(n, n)
    return (mesh, fem.FunctionSpace(mesh, 'CG', 1),
            fem.FunctionSpace(mesh, 'CG', 2))


def _table(form):
    rank, tab = form.argument_table()
    if rank == 2:
        return {(b, a): tab[b][a] for b in range(3) for a in range(3)
                if tab[b][a] is not None}
    return {b: tab[b] for b in range(3) if tab[b] is not None}


ONE = ('num', 1.0)


def test_tables_mass_and_stiffness():
    _, V1, V2 = _spaces()
    for V in (V1, V2):
        u, v = TrialFunction(V), TestFunction(V)
        a = u * v * dx
        assert a.rank == 2 and a.function_space() is V
        assert _table(a) == {(0, 0): ONE}
        assert a.degree() == 2 * V.degree
        k = inner(grad(u), grad(v)) * dx
        assert _table(k) == {(1, 1): ONE, (2, 2): ONE}
        assert k.degree() == 2 * (V.degree - 1)
        assert forms.is_symmetric_table(k.argument_table()[1])
        # the order of the factors does not matter
        assert _table(v * u * dx) == {(0, 0): ONE}
        assert _table(u.dx(0) * v.dx(1) * dx) == {(2, 1): ONE}
        assert _table(-(u.dx(1) * v) * dx) == {(0, 2): ('num', -1.0)}


def test_tables_convection_and_quotient():
    mesh, V1, V2 = _spaces()
    W = fem.VectorFunctionSpace(mesh, 'CG', 2)
    w = fem.Function(W)
    u, v = TrialFunction(V2), TestFunction(V2)
    a = dot(w, grad(u)) * v * dx
    assert _table(a) == {(0, 1): ('field', w, 0, 0), (0, 2): ('field', w, 1, 0)}
    assert a.degree() == 2 + 1 + 2
    assert not forms.is_symmetric_table(a.argument_table()[1])
    # the other orientation: u w.grad(v)
    assert _table(u * dot(w, grad(v)) * dx) == {
        (1, 0): ('field', w, 0, 0), (2, 0): ('field', w, 1, 0)}
    # grad(v / c) expands by the quotient rule; the coefficient k c / c^2
    k, c = fem.Constant(3.0), fem.Constant(2.0)
    kt, ct = ('const', k, 0), ('const', c, 0)
    coef = ('mul', kt, ('div', ct, ('powi', ct, 2)))
    a = k * dot(grad(u), grad(v / c)) * dx
    assert _table(a) == {(1, 1): coef, (2, 2): coef}
    assert a.degree() == 2
    a = k * dot(grad(u), grad(v / 4.0)) * dx
    num = ('mul', kt, ('div', ('num', 4.0), ('powi', ('num', 4.0), 2)))
    assert _table(a) == {(1, 1): num, (2, 2): num}
    # a product with a coefficient inside the gradient: the product rule
    th = fem.Function(V1)
    a = dot(grad(u), grad(th * v)) * dx
    tht = ('field', th, 0, 0)
    assert _table(a) == {(1, 1): tht, (0, 1): ('field', th, 0, 1),
                         (2, 2): tht, (0, 2): ('field', th, 0, 2)}


def test_tables_tensor_reaction_and_load():
    mesh, V1, V2 = _spaces()
    X = fem.SpatialCoordinate(mesh)
    th = fem.Function(V1)
    u, v = TrialFunction(V1), TestFunction(V1)
    D = as_vector([[1.0 + th * th, 0.5 * X[0]], [0.25, 2.0]])
    a = dot(D * grad(u), grad(v)) * dx
    tht = ('field', th, 0, 0)
    assert _table(a) == {
        (1, 1): ('add', ('num', 1.0), ('mul', tht, tht)),
        (1, 2): ('mul', ('num', 0.5), ('x', 0)),
        (2, 1): ('num', 0.25), (2, 2): ('num', 2.0)}
    assert not forms.is_symmetric_table(a.argument_table()[1])
    assert a.degree() == 2
    r = sin(X[0]) * u * v * dx
    assert _table(r) == {(0, 0): ('sin', ('x', 0))}
    assert r.degree() == 1 + 2 + 1 + 1
    f = fem.Expression('x[0]', degree=2)
    g = as_vector([X[1], fem.Constant(2.0)])
    c2 = fem.Constant(2.0)
    L = f * v * dx
    assert L.rank == 1 and _table(L) == {0: ('expr', f, 0)}
    assert L.degree() == 3
    g = as_vector([X[1], c2])
    L = dot(g, grad(v)) * dx
    assert _table(L) == {1: ('x', 1), 2: ('const', c2, 0)}
    # a term that folds to zero is dropped
    assert _table((u * v + 0.0 * u.dx(0) * v) * dx) == {(0, 0): ONE}
    # sums inside one integrand distribute, with signs
    a = ((u - 2.0 * u.dx(0)) * (v + v.dx(1))) * dx
    assert _table(a) == {(0, 0): ONE, (2, 0): ONE, (0, 1): ('num', -2.0),
                         (2, 1): ('num', -2.0)}


def test_programs_and_slots():
    mesh, V1, V2 = _spaces()
    W = fem.VectorFunctionSpace(mesh, 'CG', 2)
    w = fem.Function(W)
    u, v = TrialFunction(V2), TestFunction(V2)
    a = (-0.5 * inner(grad(u), grad(v)) - dot(w, grad(u)) * v) * dx
    rank, tab = a.argument_table()
    prog = forms.argument_program(tab, rank)
    assert prog.nout == 9 and prog.slots == [1, 2, 4, 8]
    outs = [ins[3] for ins in prog.code if ins[0] == forms.OPS['out']]
    assert outs == [1, 2, 4, 8]
    assert len(prog.fields) == 2
    L = (fem.Constant(1.0) * v.dx(1)) * dx
    rank, tab = L.argument_table()
    prog = forms.argument_program(tab, rank)
    assert prog.nout == 3 and prog.slots == [2]
    # arguments themselves never compile
    with pytest.raises(ValueError):
        forms.Program([(u * v).comps])


def test_lhs_rhs_equation():
    mesh, V1, V2 = _spaces()
    u, v = TrialFunction(V1), TestFunction(V1)
    f = fem.Constant(2.0)
    a1, a2, L1, L2 = u * v * dx, inner(grad(u), grad(v)) * dx, f * v * dx, \
        v.dx(0) * dx
    F = a1 - L1 + a2 + L2
    a, L = system(F)
    assert [(s, p) for s, p in a.terms()] == [(1.0, a1), (1.0, a2)]
    # the linear parts are negated, as UFL's rhs
    assert [(s, p) for s, p in L.terms()] == [(1.0, L1), (-1.0, L2)]
    assert lhs(F).rank == 2 and rhs(F).rank == 1
    with pytest.raises(ValueError):
        F.rank
    assert rhs(a1 + a2).terms() == []
    with pytest.raises(ValueError):
        lhs(a1 + fem.Constant(1.0) * dx(mesh))
    eq = a == L
    assert isinstance(eq, forms.Equation)
    assert eq.lhs is a and eq.rhs is L
    assert isinstance(a1 == L1, forms.Equation)
    # rank-0 forms keep Python's comparison; forms stay hashable
    m0, m1 = fem.Constant(1.0) * dx(mesh), fem.Constant(1.0) * dx(mesh)
    assert (m0 == m1) is False and (m0 == m0) is True
    assert len({a1, a2, m0, m0}) == 3
    # Functions, Constants and Expressions keep the identity comparison
    fn = fem.Function(V1)
    for obj in (fn, f, fem.Expression('x[0]', degree=1)):
        assert (obj == obj) is True and (obj == fem.Constant(2.0)) is False
        assert hash(obj) == object.__hash__(obj)


def test_quadrature_parameters():
    mesh, V1, V2 = _spaces()
    u, v = TrialFunction(V2), TestFunction(V2)
    assert (u * v * dx(degree=7)).degree() == 7
    assert (u * v * dx(metadata={'quadrature_degree': 3})).degree() == 3
    assert forms.quadrature_scheme(None, {}) == 'default'
    assert forms.quadrature_scheme(
        {'quadrature_rule': 'vertex', 'representation': 'quadrature'},
        {}) == 'vertex'
    assert forms.quadrature_scheme(None, {'quadrature_rule': 'vertex'}) \
        == 'vertex'
    with pytest.raises(ValueError):
        forms.quadrature_scheme({'quadrature_rule': 'canonical'})
    # the vertex rule gives the lumped mass: |T|/3 on the vertex rows, zero
    # edge rows (P2)
    fcp = {'quadrature_rule': 'vertex'}
    M = bref.matrix(u * v * dx, fcp).toarray()
    assert numpy.abs(M - numpy.diag(numpy.diag(M))).max() == 0.0
    lay = V2.layout
    lumped = numpy.zeros(V2.N)
    numpy.add.at(lumped, lay.cell_dofs[:, :3],
                 (mesh.cell_areas() / 3.0)[:, None])
    assert numpy.abs(numpy.diag(M) - lumped).max() < 1e-15
    assert (lumped[lay.edge_dofs] == 0.0).all()


def test_not_linear():
    mesh, V1, V2 = _spaces()
    u, v = TrialFunction(V1), TestFunction(V1)
    th = fem.Function(V1)
    bad = [
        (abs(u) * v, 'abs'), (sqrt(u) * v, 'sqrt'), (u**2 * v, r'\*\*'),
        (u**0.5 * v, r'\*\*'), (sin(u) * v, 'sin'), (v / u, '/'),
        (th / (1.0 + v) * u, '/'), (u * u * v, r'twice.*\*'),
        (v * v, r'twice.*\*'), (2.0**v * u, r'\*\*'),
        ]
    for expr, what in bad:
        with pytest.raises(ValueError, match=what):
            (expr * dx).rank
    # the test function without the trial function in a sum that has both
    with pytest.raises(ValueError, match='rank'):
        ((u * v + th * v) * dx).rank
    with pytest.raises(ValueError, match='rank'):
        ((u * v + th) * dx).rank
    with pytest.raises(ValueError, match='trial'):
        (u * th * dx).rank
    with pytest.raises(NotImplementedError, match='second'):
        grad(grad(u))


def test_out_of_scope():
    mesh, V1, V2 = _spaces()
    W = fem.VectorFunctionSpace(mesh, 'CG', 2)
    u, v = TrialFunction(V1), TestFunction(V1)
    for make in (TestFunction, TrialFunction):
        with pytest.raises(NotImplementedError, match='vector'):
            make(W)
        with pytest.raises(NotImplementedError, match='component'):
            make(W.sub(0))
        with pytest.raises(NotImplementedError, match='mixed'):
            make(fem.MixedFunctionSpace(
                mesh, fem.VectorElement('Lagrange', 'triangle', 2)
                * fem.FiniteElement('Lagrange', 'triangle', 1)))
    # test and trial functions of different spaces, or of different meshes
    with pytest.raises(NotImplementedError, match='different spaces'):
        (TrialFunction(V2) * v * dx).rank
    other = fem.FunctionSpace(fem.UnitSquareMesh(2, 2), 'CG', 1)
    for meet in (lambda: TrialFunction(other) * v,
                 lambda: inner(grad(TrialFunction(other)), grad(v)),
                 lambda: dot(grad(TrialFunction(other)), grad(v)),
                 lambda: TrialFunction(other) + v):
        with pytest.raises(NotImplementedError, match='different meshes'):
            meet()
    # (a FIELD of another mesh stays the ValueError it was)
    with pytest.raises(ValueError, match='two different meshes'):
        fem.Function(other) * v
    with pytest.raises(NotImplementedError, match='different spaces'):
        (u * v * dx + TrialFunction(V2) * TestFunction(V2) * dx).arguments()
    # Neumann / Robin terms
    with pytest.raises(NotImplementedError, match='contribution map'):
        fem.Constant(1.0) * v * ds
    with pytest.raises(NotImplementedError, match='contribution map'):
        u * v * ds(mesh)
    with pytest.raises(NotImplementedError, match='dS'):
        u * v * fem.dS
    with pytest.raises(NotImplementedError, match='dS'):
        fem.dS(mesh)
    a = u * v * dx
    for name in ('derivative', 'action', 'adjoint'):
        with pytest.raises(NotImplementedError, match=name):
            getattr(fem, name)(a, fem.Function(V1))


def test_strips_refused(monkeypatch):
    from flow_amd import parallel
    from flow_amd.fem import ops
    mesh, V1, V2 = _spaces()
    u, v = TrialFunction(V1), TestFunction(V1)
    a, L = inner(grad(u), grad(v)) * dx, fem.Constant(1.0) * v * dx
    bc = fem.DirichletBC(V1, 0.0, 'on_boundary')
    # (built before the strips are switched on: no kernel runs in __init__)
    A = ops.Matrix.__new__(ops.Matrix)
    A.layout, A.kind = V1.layout, 0
    x = fem.Function.__new__(fem.Function)
    monkeypatch.setattr(parallel, 'active', lambda: True)
    calls = [
        lambda: fem.assemble(a), lambda: fem.assemble(L),
        lambda: fem.assemble(a + a), lambda: fem.assemble(rhs(a - L)),
        lambda: fem.assemble_system(a, L, [bc]),
        lambda: fem.assemble_system(a, None),
        lambda: fem.solve(a == L, x, [bc]),
        lambda: bc.apply(A), lambda: bc.apply(A, x), lambda: bc.apply(x),
        lambda: A * x, lambda: A @ x,
        ]
    for call in calls:
        with pytest.raises(NotImplementedError, match='on strips'):
            call()


def test_reference_evaluator_closed_forms():
    # P1 stiffness of the right triangle (0,0), (1,0), (0,1)
    mesh = fem.UnitSquareMesh(1, 1)
    V = fem.FunctionSpace(mesh, 'CG', 1)
    u, v = TrialFunction(V), TestFunction(V)
    _, Ke = bref.element_tensors(inner(grad(u), grad(v)) * dx)
    P = mesh.points[mesh.cell_vertices]
    for c in range(mesh.num_cells()):
        # gradients of the barycentric coordinates from the vertices
        B = numpy.linalg.inv(numpy.column_stack([numpy.ones(3), P[c]]))[1:]
        area = mesh.cell_areas()[c]
        assert numpy.abs(Ke[c] - area * B.T.dot(B)).max() < 1e-14
    right = [c for c in range(mesh.num_cells())
             if numpy.allclose(numpy.sort(numpy.linalg.norm(
                 P[c] - P[c].mean(axis=0), axis=1)), numpy.sort(numpy.linalg.norm(
                     numpy.array([[0, 0], [1, 0], [0, 1.0]]) - 1 / 3.0, axis=1)))]
    assert right
    ev = numpy.sort(numpy.linalg.eigvalsh(Ke[right[0]]))
    assert numpy.abs(ev - [0.0, 0.5, 1.5]).max() < 1e-14
    # P2 mass: the row sums are int phi_i (0 at vertices, |T|/3 on edges)
    mesh, V1, V2 = _spaces(4)
    u, v = TrialFunction(V2), TestFunction(V2)
    M = bref.matrix(u * v * dx)
    b = bref.vector(fem.Constant(1.0) * v * dx)
    assert numpy.abs(numpy.asarray(M.sum(axis=1)).ravel() - b).max() < 1e-15
    exact = numpy.zeros(V2.N)
    numpy.add.at(exact, V2.layout.cell_dofs[:, 3:],
                 (mesh.cell_areas() / 3.0)[:, None])
    assert numpy.abs(b - exact).max() < 1e-15
    assert abs(M.sum() - 1.0) < 1e-14
    assert abs(M - M.T).max() < 1e-16
    # a rank-1 form with a gradient: int d(phi_i)/dx sums to zero inside
    L = bref.vector(v.dx(0) * dx)
    assert abs(L.sum()) < 1e-14
