# -*- coding: utf-8 -*-
'''
Test and trial functions on vector spaces (forms.vector_arguments), host
side: the switch, the argument leaves, block tables and their symmetry, lhs /
rhs, the tensor helpers, the refusals, the unchanged programs of scalar forms
and the C ABI of the new entry points.  No device.
'''
import ctypes
import os

import numpy
import pytest

from flow_amd import fem, _hip
from flow_amd.fem import forms
from flow_amd.fem import (
    TestFunction, TrialFunction, dx, ds, dot, inner, grad, div, curl, sym, tr,
    transpose, Identity, outer, as_vector, lhs, rhs, system, conditional, gt,
    SpatialCoordinate, sin,
    )

import newton_reference as nref


@pytest.fixture()
def on():
    with fem.vector_arguments(True):
        yield


def _spaces(degree=1):
    mesh = fem.UnitSquareMesh(3, 2)
    return (mesh, fem.VectorFunctionSpace(mesh, 'CG', degree),
            fem.FunctionSpace(mesh, 'CG', degree))


def test_switch():
    mesh, W, V = _spaces()
    assert forms.vector_arguments.enabled is False
    for make in (TestFunction, TrialFunction):
        with pytest.raises(NotImplementedError, match='vector'):
            make(W)
    with fem.vector_arguments(True) as sw:
        assert sw.previous is False and forms.vector_arguments.enabled is True
        assert TestFunction(W).shape == (2,)
        with fem.vector_arguments(False) as inner_:
            assert inner_.previous is True
            with pytest.raises(NotImplementedError, match='vector'):
                TestFunction(W)
        assert forms.vector_arguments.enabled is True
    assert forms.vector_arguments.enabled is False
    # called, not entered: switched at once, for the process
    sw = fem.vector_arguments(True)
    try:
        assert sw.previous is False and forms.vector_arguments.enabled is True
        assert fem.vector_arguments(True).previous is True
    finally:
        fem.vector_arguments(False)
    with pytest.raises(NotImplementedError, match='vector'):
        TestFunction(W)


def test_leaves_and_shapes(on):
    for degree in (1, 2):
        mesh, W, V = _spaces(degree)
        v, u = TestFunction(W), TrialFunction(W)
        assert v.shape == (2,) and v.deg == degree and v.mesh is mesh
        assert v.comps == [('arg', 0, 0, W, 0), ('arg', 0, 0, W, 1)]
        assert u.comps == [('arg', 1, 0, W, 0), ('arg', 1, 0, W, 1)]
        assert u[1].comps == ('arg', 1, 0, W, 1) and u[1].shape == ()
        g = grad(u)
        assert g.shape == (2, 2) and g.deg == degree - 1
        assert g.comps[1][0] == ('arg', 1, 1, W, 1)
        assert g.comps[0][1] == ('arg', 1, 2, W, 0)
        assert u.dx(1).comps[0] == ('arg', 1, 2, W, 0)
        assert div(u).shape == () and curl(u).shape == ()
        assert curl(u).comps == ('sub', ('arg', 1, 1, W, 1),
                                 ('arg', 1, 2, W, 0))
        with pytest.raises(NotImplementedError, match='second derivatives'):
            grad(u[0]).dx(0)
        # the scalar leaf keeps its 4-tuple
        assert TestFunction(V).comps == ('arg', 0, 0, V)
        a = inner(grad(u), grad(v)) * dx
        assert a.rank == 2 and set(a.arguments()) == {0, 1}
        assert a.arguments()[0] is W and a.function_space() is W
        assert forms.has_leaf(a.integrand.comps, 'arg')
        assert (dot(fem.Constant((1.0, 2.0)), v) * dx).rank == 1
        keys = forms.extract_arguments((u[1].dx(0) * v[0]).comps)
        assert list(keys) == [((0, 0), (1, 1))]


def test_block_tables(on):
    mesh, W, V = _spaces(2)
    v, u = TestFunction(W), TrialFunction(W)
    vs, us = TestFunction(V), TrialFunction(V)
    rank, t = (inner(grad(u), grad(v)) * dx).argument_table()
    _, ts = (inner(grad(us), grad(vs)) * dx).argument_table()
    assert rank == 2 and len(t) == 2 and len(t[0]) == 2
    assert t[0][0] == ts and t[1][1] == ts
    assert t[0][1] is None and t[1][0] is None
    assert forms.is_symmetric_table(t)
    _, tm = (dot(u, v) * dx).argument_table()
    assert tm[0][0] == (us * vs * dx).argument_table()[1] == tm[1][1]
    assert tm[0][1] is None and tm[1][0] is None
    # grad-div: v_0,x u_1,y in block (0, 1) and its mirror
    _, t = (div(u) * div(v) * dx).argument_table()
    one = ('num', 1.0)
    assert t[0][1] == [[None] * 3, [None, None, one], [None] * 3]
    assert t[1][0] == [[None] * 3, [None] * 3, [None, one, None]]
    assert t[0][0][1][1] == one and t[1][1][2][2] == one
    assert forms.is_symmetric_table(t)
    assert forms.block_items(t, 2)[1][0] == 1 and len(
        forms.block_items(t, 2)) == 4
    # elasticity
    mu, lam = fem.Constant(1.3), fem.Constant(0.7)

    def eps(w):
        return sym(grad(w))

    def sigma(w):
        return 2.0 * mu * eps(w) + lam * tr(eps(w)) * Identity(2)

    a = inner(sigma(u), eps(v)) * dx
    assert a.rank == 2 and a.degree() == 2
    _, t = a.argument_table()
    assert all(t[r][s] is not None for r in range(2) for s in range(2))
    assert forms.is_symmetric_table(t)
    # a first-order term is not symmetric
    w = fem.Function(W)
    c = dot(dot(grad(u), w), v) * dx
    _, t = c.argument_table()
    assert t[0][1] is None and t[1][0] is None
    assert t[0][0][0][1] == ('field', w, 0, 0)
    assert t[1][1][0][2] == ('field', w, 1, 0)
    assert not forms.is_symmetric_table(t)
    # rank 1, one component only, and conditional branches
    rank, t = (v[1] * dx).argument_table()
    assert rank == 1 and t[0] is None and t[1] == [('num', 1.0), None, None]
    X = SpatialCoordinate(mesh)
    rank, t = (dot(conditional(gt(X[0], 0.5), u, 2.0 * u), v)
               * dx).argument_table()
    assert rank == 2 and t[0][0][0][0][0] == 'cond' and t[0][1] is None
    # one program per present block: the scalar form's bytes
    ps = forms.argument_programs(ts, 2)
    _, t = (inner(grad(u), grad(v)) * dx).argument_table()
    for p, block in forms.block_items(t, 2):
        assert p in (0, 3)
        pb = forms.argument_programs(block, 2)
        assert len(pb) == 1 and pb[0].signature() == ps[0].signature()
        assert pb[0].slots == ps[0].slots and pb[0].nout == 9


def test_lhs_rhs(on):
    mesh, W, V = _spaces(1)
    v, u = TestFunction(W), TrialFunction(W)
    f = fem.Constant((1.0, -2.0))
    k = fem.Constant(3.0)
    F = (k * dot(u, v) + inner(grad(u), grad(v)) - dot(f, v)) * dx
    with pytest.raises(ValueError, match='differ in rank'):
        F.argument_table()
    a, L = system(F)
    assert a.rank == 2 and L.rank == 1
    assert lhs(F).arguments()[1] is W
    _, ta = a.terms()[0][1].argument_table()
    assert ta[0][0][0][0] == ('const', k, 0) and ta[0][0][1][1] == ('num', 1.0)
    assert ta[0][1] is None
    (sign, part), = L.terms()
    assert sign == -1.0
    _, tl = part.argument_table()
    assert tl[0] == [('neg', ('const', f, 0)), None, None]
    assert tl[1] == [('neg', ('const', f, 1)), None, None]
    # a sum of parts of both ranks
    G = inner(grad(u), grad(v)) * dx - dot(f, v) * dx
    assert lhs(G).rank == 2 and rhs(G).rank == 1
    with fem.facet_arguments(True):
        H = G + dot(u, v) * ds - dot(f, v) * ds
        assert len(lhs(H).terms()) == 2 and len(rhs(H).terms()) == 2
        assert (dot(f, v) * ds).integral_type == 'exterior_facet'
    with pytest.raises(NotImplementedError, match='facet_arguments'):
        dot(f, v) * ds


def _values(expr, leaves):
    return numpy.array([nref.eval_tree(t, leaves)[0]
                        for t in expr.scalar_trees()]).reshape(expr.shape)


def test_tensor_helpers():
    mesh, W, V = _spaces(2)
    w, z = fem.Function(W), fem.Function(W)
    X = SpatialCoordinate(mesh)
    A = grad(w) + outer(X, z)
    b = as_vector([sin(X[0]), 2.0 + X[1]])
    leaves = nref.Leaves(1)
    Av, bv = _values(A, leaves), _values(b, leaves)
    zv = _values(fem.as_vector([z[0], z[1]]), leaves)
    assert A.shape == (2, 2)
    for got, ref in ((sym(A), 0.5 * (Av + Av.T)), (transpose(A), Av.T),
                     (A.T, Av.T), (tr(A), numpy.trace(Av)),
                     (Identity(2), numpy.eye(2)),
                     (outer(b, z), numpy.outer(bv, zv)),
                     (2.0 * A - Identity(2), 2.0 * Av - numpy.eye(2)),
                     (tr(A) * Identity(2) + sym(A),
                      numpy.trace(Av) * numpy.eye(2) + 0.5 * (Av + Av.T)),
                     (inner(sym(A), A.T), (0.5 * (Av + Av.T) * Av.T).sum()),
                     (dot(A, b), Av.dot(bv)), (dot(b, A), bv.dot(Av))):
        assert numpy.allclose(_values(got, leaves), ref, rtol=1e-14, atol=0)
    # degrees: UFL's rules
    assert sym(grad(w)).deg == 1 and tr(grad(w)).deg == 1
    assert transpose(grad(w)).deg == 1 and Identity(2).deg == 0
    assert outer(w, X).deg == 3 and Identity(2).mesh is None
    assert (tr(grad(w)) * Identity(2)).deg == 1
    for bad in (lambda: sym(w), lambda: tr(X), lambda: transpose(w),
                lambda: outer(A, w), lambda: Identity(3)):
        with pytest.raises(ValueError):
            bad()


def test_refusals(on):
    mesh, W, V = _spaces(1)
    v, u = TestFunction(W), TrialFunction(W)
    vs, us = TestFunction(V), TrialFunction(V)
    for make in (TestFunction, TrialFunction):
        with pytest.raises(NotImplementedError, match='component view'):
            make(W.sub(0))
        with pytest.raises(NotImplementedError, match='mixed'):
            make(fem.FunctionSpace(mesh, fem.VectorElement('P', 'triangle', 2)
                                   * fem.FiniteElement('P', 'triangle', 1)))
    # a vector test function with a scalar trial function, and the reverse
    for form in (us * v[0] * dx, u[1] * vs * dx,
                 dot(u, TestFunction(fem.VectorFunctionSpace(mesh, 'CG', 2)))
                 * dx):
        with pytest.raises(NotImplementedError, match='different spaces'):
            form.rank
    with pytest.raises(NotImplementedError, match='different spaces'):
        forms.argument_table((us * v[0]).comps)
    with pytest.raises(ValueError, match='not linear'):
        (dot(u, u) * v[0] * dx).rank
    # derivative with respect to a vector Function, the nonlinear solve
    w = fem.Function(W)
    with pytest.raises(NotImplementedError, match='vector'):
        fem.derivative(dot(w, w) * dx, w)
    with pytest.raises(NotImplementedError, match='vector'):
        fem.derivative(dot(w, v) * dx, w)
    with pytest.raises(NotImplementedError, match='vector space'):
        fem.solve((inner(grad(w), grad(v)) + dot(w, v)) * dx == 0, w)
    # Eigenmodes
    with pytest.raises(NotImplementedError, match='vector space'):
        fem.eigen._check_forms(inner(grad(u), grad(v)) * dx, dot(u, v) * dx,
                               False)


def test_strips_refused(on, monkeypatch):
    from flow_amd import parallel
    from flow_amd.fem import ops
    mesh, W, V = _spaces(1)
    u, v = TrialFunction(W), TestFunction(W)
    a = inner(sym(grad(u)), sym(grad(v))) * dx + div(u) * div(v) * dx
    L = dot(fem.Constant((1.0, 2.0)), v) * dx
    bcs = [fem.DirichletBC(W, (0.0, 0.0), 'on_boundary'),
           fem.DirichletBC(W.sub(1), 1.0, 'on_boundary')]
    # (built before the strips are switched on: no kernel runs in __init__)
    A = ops.Matrix.__new__(ops.Matrix)
    A.layout, A.kind = W.layout, 2
    x = fem.Function.__new__(fem.Function)
    monkeypatch.setattr(parallel, 'active', lambda: True)
    calls = [
        lambda: fem.assemble(a), lambda: fem.assemble(L),
        lambda: fem.assemble(a + a), lambda: fem.assemble(rhs(a - L)),
        lambda: fem.assemble_system(a, L, bcs),
        lambda: fem.assemble_system(a, None),
        lambda: fem.solve(a == L, x, bcs),
        lambda: bcs[0].apply(A), lambda: bcs[1].apply(A, x),
        lambda: bcs[1].apply(x), lambda: A * x, lambda: A @ x,
        ]
    with fem.facet_arguments(True):
        calls.append(lambda: fem.assemble(dot(u, v) * ds))
        calls.append(lambda: fem.assemble(v[0] * ds))
        for call in calls:
            with pytest.raises(NotImplementedError, match='on strips'):
                call()


def test_scalar_programs_unchanged():
    mesh, W, V = _spaces(2)
    w = fem.Function(W)
    c = fem.Constant(0.3)

    def programs():
        v, u = TestFunction(V), TrialFunction(V)
        X = SpatialCoordinate(mesh)
        out = []
        for form in ((c * inner(grad(u), grad(v)) + dot(w, grad(u)) * v
                      + sin(X[0]) * u * v) * dx,
                     (1.0 + X[1]) * v * dx + c * v.dx(0) * dx):
            for _, part in form.terms():
                rank, table = part.argument_table()
                out.append((rank, table))
                out += [(p.signature(), p.slots, p.nout, p.constant_values())
                        for p in forms.argument_programs(table, rank)]
        return out

    off = programs()
    with fem.vector_arguments(True):
        assert programs() == off
    assert programs() == off


def test_new_symbols_resolve():
    '''The entry points exist in the built library with the argument types
    _hip.py declares (and the header names).'''
    names = ('flow_form_block_matrix', 'flow_form_block_vector',
             'flow_bc_symmetric_blocks')
    for name in names:
        assert name in _hip.SYMBOLS
    lib = _hip.load_library()
    for name in names:
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int
        assert list(fn.argtypes) == _hip.SYMBOLS[name]
    assert len(_hip.SYMBOLS['flow_form_block_matrix']) == 9
    assert _hip.SYMBOLS['flow_form_block_matrix'][7] is ctypes.c_size_t
    assert len(_hip.SYMBOLS['flow_form_block_vector']) == 8
    assert len(_hip.SYMBOLS['flow_bc_symmetric_blocks']) == 10
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)),
                               '..', 'include', 'flow_hip.h')).read()
    for name in names:
        assert 'int %s(' % name in header
    assert lib.flow_abi_version() == _hip.ABI_VERSION
