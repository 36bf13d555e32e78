# -*- coding: utf-8 -*-
'''
derivative() with respect to a Function of a vector space and the block
Newton job lists (forms.vector_derivatives, ops.newton_jobs), host side: the
switch, the vector leaf rule, derived Jacobians against Jacobians written by
hand and against central differences, which jobs fuse, the refusals and the C
ABI of flow_form_block_newton.  No device.
'''
import ctypes
import os
import re

import numpy
import pytest

from flow_amd import fem, _hip
from flow_amd.fem import forms, ops
from flow_amd.fem import (
    TestFunction, TrialFunction, dx, ds, dot, inner, grad, derivative,
    )

import newton_reference as nref
import vector_form_reference as vref
import vector_newton_reference as vnref


@pytest.fixture()
def on():
    with fem.vector_arguments(True), fem.facet_arguments(True), \
            fem.vector_derivatives(True):
        yield


def _spaces(degree=1):
    mesh = fem.UnitSquareMesh(3, 2)
    return (mesh, fem.VectorFunctionSpace(mesh, 'CG', degree),
            fem.FunctionSpace(mesh, 'CG', degree))


def _refused_when_off(W):
    w, v = fem.Function(W), TestFunction(W)
    with pytest.raises(NotImplementedError, match='vector'):
        derivative(dot(w, w) * dx, w)
    with pytest.raises(NotImplementedError, match='vector'):
        derivative(dot(w, v) * dx, w)
    with pytest.raises(NotImplementedError, match='vector space'):
        fem.solve((inner(grad(w), grad(v)) + dot(w, v)) * dx == 0, w)


def test_switch():
    mesh, W, V = _spaces()
    assert forms.vector_derivatives.enabled is False
    assert fem.vector_derivatives is forms.vector_derivatives
    with fem.vector_arguments(True):
        _refused_when_off(W)
        with fem.vector_derivatives(True) as sw:
            assert sw.previous is False
            assert forms.vector_derivatives.enabled is True
            w = fem.Function(W)
            assert derivative(dot(w, TestFunction(W)) * dx, w).rank == 2
            with fem.vector_derivatives(False) as inner_:
                assert inner_.previous is True
                _refused_when_off(W)
            assert forms.vector_derivatives.enabled is True
        assert forms.vector_derivatives.enabled is False
        _refused_when_off(W)
        # called, not entered: switched at once, for the process
        sw = fem.vector_derivatives(True)
        try:
            assert sw.previous is False
            assert fem.vector_derivatives(True).previous is True
        finally:
            fem.vector_derivatives(False)
        _refused_when_off(W)
    # on, but without vector_arguments: the message names the missing switch
    w = fem.Function(W)
    with fem.vector_derivatives(True):
        with pytest.raises(NotImplementedError, match=r'vector_arguments\(True\)'):
            derivative(dot(w, w) * dx, w)
    assert forms.vector_derivatives.enabled is False


def test_leaf_rule_and_ranks(on):
    for degree in (1, 2):
        mesh, W, V = _spaces(degree)
        w = fem.Function(W)
        v, du = TestFunction(W), TrialFunction(W)
        # the leaf rule, on the trees
        assert forms.s_gateaux(('field', w, 1, 2), w, 1, W) \
            == ('arg', 1, 2, W, 1)
        assert forms.s_gateaux(('field', fem.Function(W), 1, 0), w, 1, W) \
            == forms.ZERO
        # a residual: the table of dot(du, v)*dx
        J = derivative(dot(w, v) * dx, w)
        assert J.rank == 2 and J.arguments()[1] is W
        assert J.argument_table() == (dot(du, v) * dx).argument_table()
        assert J.derived_from is not None
        # du given
        assert derivative(dot(w, v) * dx, w, du).argument_table() \
            == J.argument_table()
        # an energy: rank 1, twice the bilinear form
        E = 0.5 * inner(grad(w), grad(w)) * dx
        dE = derivative(E, w)
        assert dE.rank == 1 and dE.arguments()[0] is W
        assert derivative(E, w, v).rank == 1
        d2E = derivative(dE, w)
        assert d2E.rank == 2
        A = vref.matrix(d2E).toarray()
        B = vref.matrix(inner(grad(du), grad(v)) * dx).toarray()
        assert numpy.abs(A - B).max() <= 1e-14 * numpy.abs(B).max()
        ta = d2E.argument_table()[1]
        tb = (inner(grad(du), grad(v)) * dx).argument_table()[1]
        # ... and its table: the same terms, with the same values
        leaves = nref.Leaves(1)
        for r in range(2):
            for s in range(2):
                assert (ta[r][s] is None) == (tb[r][s] is None)
                for b in range(3):
                    for a in range(3):
                        if ta[r][s] is None or tb[r][s][b][a] is None:
                            assert ta[r][s] is None or ta[r][s][b][a] is None
                            continue
                        assert nref.eval_tree(ta[r][s][b][a], leaves)[0] \
                            == nref.eval_tree(tb[r][s][b][a], leaves)[0] == 1.0
        # signs, parts that do not depend on w, the degree rule, ds parts
        f = fem.Constant((1.0, 2.0))
        G = dot(w, w) * dot(w, v) * dx - dot(f, v) * dx - dot(w, v) * ds
        dG = derivative(G, w)
        assert [s for s, _ in dG.terms()] == [1.0, -1.0]
        parts = [p for _, p in dG.terms()]
        assert parts[0].integrand.deg == 4 * degree
        assert parts[1].integral_type == 'exterior_facet'
        assert parts[0].derived_from is G.terms()[0][1]


def test_derived_against_hand_written(on):
    '''vref of derivative(F, u) against vref of the Jacobian written by hand,
    entrywise relative to max|entry|, below 1e-12 -- both at the quadrature
    degree of the residual's part (a derived part keeps it; the estimate of a
    hand-written non-polynomial Jacobian differs).  Measured on the CPU:
    at most 4e-16.'''
    for mesh in (fem.UnitSquareMesh(4, 3),):
        for degree in (1, 2):
            W = fem.VectorFunctionSpace(mesh, 'CG', degree)
            for name, u, F, J in vnref.residuals(W):
                q = {'quadrature_degree': F.terms()[0][1].degree()}
                Jd = derivative(F, u)
                A = vref.matrix(Jd, q).toarray()
                B = vref.matrix(J, q).toarray()
                e = numpy.abs(A - B).max() / numpy.abs(B).max()
                print('P%d %-16s derived vs hand-written J %.2e'
                      % (degree, name, e))
                assert e < 1e-12


def test_directional_derivative(on):
    '''Burgers is quadratic in u, so (F(u + h d) - F(u - h d)) / 2h IS J d up
    to rounding.  Each of the two residuals carries a rounding error of a few
    eps max|F| (sums of some tens of products per entry), the difference
    quotient divides it by h = 1e-3: the bound is 100 eps max|F| / h, the
    factor 100 for the length of the sums and the cancellation between
    element contributions.  Measured on the CPU: at most 3 eps max|F| / h.'''
    h = 1.0e-3
    eps = numpy.finfo(float).eps
    mesh = fem.UnitSquareMesh(4, 3)
    for degree in (1, 2):
        W = fem.VectorFunctionSpace(mesh, 'CG', degree)
        u = vnref.state(W)
        F, _ = vnref.burgers(W, u)
        d = numpy.random.RandomState(3).uniform(-1.0, 1.0, W.size())
        Jd = vref.matrix(derivative(F, u)).dot(d)
        fd = vnref.central_difference(F, u, d, h)
        scale = eps * numpy.abs(vref.vector(F)).max() / h
        e = numpy.abs(Jd - fd).max()
        print('P%d |J d - central difference| = %.2e = %.1f eps max|F| / h'
              % (degree, e, e / scale))
        assert e < 100.0 * scale


def test_newton_jobs(on):
    mesh = fem.UnitSquareMesh(4, 3)
    for degree in (1, 2):
        W = fem.VectorFunctionSpace(mesh, 'CG', degree)
        jobs = {}
        for name, u, F, J in vnref.residuals(W):
            jobs[name] = ops.newton_jobs(derivative(F, u), F)
            pair = ops.newton_jobs(derivative(F, u), F, fuse=False)
            assert not any(j[0] == 'newton' for j in pair)
            assert not ops.block_jobs_fused(pair)
        for name in ('burgers', 'forchheimer'):
            kinds = [(j[0], j[7]) for j in jobs[name]]
            # both rows fuse, the diagonal block first; one call
            assert kinds == [('newton', 0), ('matrix', 1), ('newton', 3),
                             ('matrix', 2)], kinds
            assert set(j[8] for j in jobs[name]) == {(0, 0)}
            assert all(j[3].nout == forms.NEWTON_SLOTS
                       for j in jobs[name] if j[0] == 'newton')
            assert ops.block_jobs_fused(jobs[name])
        # St. Venant-Kirchhoff: no combined program fits
        kinds = set(j[0] for j in jobs['kirchhoff'])
        assert kinds == {'matrix', 'vector'}
        assert not ops.block_jobs_fused(jobs['kirchhoff'])
        assert set(j[8] for j in jobs['kirchhoff']) == {(0, None), (None, 0)}
        # ds parts are never fused
        kinds = [j[0] for j in jobs['traction robin']]
        assert kinds.count('newton') == 2 \
            and kinds.count('facet_matrix') == 2 \
            and kinds.count('facet_vector') == 4
        assert ops.block_jobs_fused(jobs['traction robin'])
        # a source term written as a part of its own needs 'vector' jobs
        u = vnref.state(W)
        F, _ = vnref.burgers(W, u)
        G = F - dot(fem.Constant((1.0, 0.0)), TestFunction(W)) * dx
        extra = ops.newton_jobs(derivative(G, u), G)
        assert [j[0] for j in extra].count('vector') == 2
        assert not ops.block_jobs_fused(extra)
    # the scratch the entry point asks for (include/flow_hip.h)
    assert ops._block_newton_scratch(
        ['newton', 'matrix', 'newton', 'matrix'], [0, 1, 3, 2], 3, 10) \
        == 4 * 90 + 2 * 30
    assert ops._block_newton_scratch(
        ['matrix', 'matrix', 'vector'], [0, 0, 1], 6, 10) == 360 + 60 + 360
    assert ops._block_newton_scratch(
        ['vector', 'vector'], [1, 1], 3, 10) == 30 + 30


def test_refusals(on):
    mesh, W, V = _spaces(1)
    w, v, du = fem.Function(W), TestFunction(W), TrialFunction(W)
    F = dot(w, w) * dot(w, v) * dx
    # a component view, a mixed space
    # (no Function lives on a view or a mixed space: the space is put there)
    wc = fem.Function(W)
    wc._V = W.sub(0)
    with pytest.raises(NotImplementedError, match='component'):
        derivative(F, wc)
    M = fem.FunctionSpace(mesh, fem.VectorElement('P', 'triangle', 2)
                          * fem.FiniteElement('P', 'triangle', 1))
    wm = fem.Function(W)
    wm._V = M
    with pytest.raises(NotImplementedError, match='mixed'):
        derivative(F, wm)
    # a bilinear form
    with pytest.raises(NotImplementedError, match='rank-3'):
        derivative(dot(w, w) * dot(du, v) * dx, w)
    # arguments of another space than u's
    W2 = fem.VectorFunctionSpace(mesh, 'CG', 2)
    with pytest.raises(ValueError, match='different spaces'):
        derivative(dot(w, w) * dot(w, TestFunction(W2)) * dx, w)
    # ... a scalar Function in a form on W included
    s = fem.Function(V)
    with pytest.raises(ValueError, match='different spaces'):
        derivative(s * s * dot(w, v) * dx, s)
    # a form that does not depend on u
    with pytest.raises(ValueError, match='does not depend'):
        derivative(F, fem.Function(W))
    # du of the wrong number, of a scalar space
    with pytest.raises(ValueError, match='du must be'):
        derivative(F, w, v)
    with pytest.raises(ValueError, match='du must be'):
        derivative(F, w, TrialFunction(V))
    # the scalar derivative is what it was
    sv = TestFunction(V)
    assert derivative(s**3 * sv * dx, s).argument_table()[1][0][0] is not None
    # solve: what is not a residual in u
    with pytest.raises(ValueError, match='does not depend'):
        fem.solve(dot(fem.Function(W), v) * dx == 0, w)


def test_c_abi():
    name = 'flow_form_block_newton'
    assert name in _hip.SYMBOLS
    args = _hip.SYMBOLS[name]
    assert len(args) == 12
    assert args[7] is ctypes.c_size_t and args[9] is ctypes.c_size_t
    lib = _hip.load_library()
    assert list(getattr(lib, name).argtypes) == args
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)),
                               '..', 'include', 'flow_hip.h')).read()
    decl = re.search(r'int %s\(([^;]*)\);' % name, header).group(1)
    assert len(decl.split(',')) == 12
    for k, v in ops._BLOCK_KINDS.items():
        assert int(re.search(r'#define FLOW_BLOCK_%s (\d+)' % k.upper(),
                             header).group(1)) == v
