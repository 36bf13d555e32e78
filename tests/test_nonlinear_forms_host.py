# -*- coding: utf-8 -*-
'''
derivative(), F == 0 and the Newton program on the host (flow_amd/fem/
forms.py, the parameter handling of ops.solve): Gateaux derivatives against
central differences of the numpy evaluator, exact cases, argument numbering,
equations, every refusal that needs no device, common-subtree sharing through
a numpy interpreter of the instruction stream, and Newton's method with the
evaluator's matrices and a sparse LU.  No GPU.
'''
import numpy
import pytest

from flow_amd import fem, _hip
from flow_amd.fem import (
    TestFunction, TrialFunction, dx, ds, dot, inner, grad, derivative, forms,
    )

import bilinear_reference as bref
import newton_reference as nref


def _meshes():
    return [fem.UnitSquareMesh(12, 9),
            fem.karman_channel(60, 14, fitted=True),
            fem.karman_channel_graded(lcar=1.0e-2)]


def _spaces(n=3):
    mesh = fem.UnitSquareMesh(n, n)
    return (mesh, fem.FunctionSpace(mesh, 'CG', 1),
            fem.FunctionSpace(mesh, 'CG', 2))


def test_derivative_against_central_differences():
    '''J(u) w, J = derivative(F, u) assembled by the host evaluator, against
    (F(u + e w) - F(u - e w)) / 2e of the same evaluator on the unextracted
    trees, e = 1e-6 |u|_inf, w random in [-1, 1]; max-norm relative to
    |J w|_inf.  Central differences in fp64 carry O(e^2) + O(eps/e), about
    1e-10 here, times the third derivative along w (w is rough: |grad w| ~
    1/h, which the minimal-surface residual sees).  Measured, largest over the
    three meshes and P1 / P2: quasilinear 9.4e-11, minimal surface 6.6e-07
    (fitted channel, P2; 1.2e-08 .. 6.5e-08 elsewhere), exp 1.8e-10, abs
    1.6e-10, power 1.5 2.3e-10, sin convection 1.0e-10, field / Constant /
    Expression 2.9e-10.  The bound is a decade above the largest, 7e-6; a
    wrong or missing chain-rule term shows as an O(1) error.'''
    worst = {}
    for m, mesh in enumerate(_meshes()):
        for k in (1, 2):
            V = fem.FunctionSpace(mesh, 'CG', k)
            u = nref.state(V)
            w = numpy.random.RandomState(5).uniform(-1.0, 1.0, V.N)
            eps = 1.0e-6 * numpy.abs(u.array()).max()
            for name, F in nref.residuals(mesh, V, u):
                J = derivative(F, u)
                assert J.rank == 2
                Jw = bref.matrix(J).dot(w)
                fd = nref.central_difference(F, u, w, eps)
                e = numpy.abs(Jw - fd).max() / numpy.abs(Jw).max()
                print('mesh %d P%d %-28s %.2e' % (m, k, name, e))
                worst[name] = max(worst.get(name, 0.0), e)
    print(worst)
    assert len(worst) == 7
    assert max(worst.values()) < 7.0e-6


def _table_values(form, leaves):
    rank, tab = form.argument_table()
    if rank == 2:
        return {(b, a): nref.eval_tree(tab[b][a], leaves) for b in range(3)
                for a in range(3) if tab[b][a] is not None}
    return {b: nref.eval_tree(tab[b], leaves) for b in range(3)
            if tab[b] is not None}


def _same_tables(f, g, tol=1e-14):
    leaves = nref.Leaves(50, seed=3)
    tf, tg = _table_values(f, leaves), _table_values(g, leaves)
    assert sorted(tf) == sorted(tg)
    for key in tf:
        assert numpy.abs(tf[key] - tg[key]).max() \
            <= tol * numpy.abs(tg[key]).max(), key


def test_exact_cases():
    mesh, V1, V2 = _spaces(4)
    for V in (V1, V2):
        u = nref.state(V)
        v, du = TestFunction(V), TrialFunction(V)
        # the cubic: the same table as the hand-written linearisation
        J = derivative(u**3 * v * dx, u)
        _same_tables(J, 3 * u**2 * du * v * dx)
        assert J.degree() == 4 * V.degree
        # a form linear in u reproduces the bilinear form it came from
        W = fem.VectorFunctionSpace(mesh, 'CG', 2)
        w = fem.Function(W)
        w.set_array(numpy.concatenate([1.0 + W.layout.dof_coords[:, 0],
                                       W.layout.dof_coords[:, 1]**2]))
        X = fem.SpatialCoordinate(mesh)

        def a(t):
            return ((1.0 + X[0]**2) * dot(grad(t), grad(v))
                    + dot(w, grad(t)) * v + fem.sin(X[1]) * t * v) * dx
        A = bref.matrix(derivative(a(u), u)).toarray()
        ref = bref.matrix(a(du)).toarray()
        assert numpy.abs(A - ref).max() <= 1e-14 * numpy.abs(ref).max()
        # energy -> Poisson residual -> stiffness, arguments numbered 0 then 1
        f = fem.Expression('1.0 + x[0]*x[1]', degree=2)
        E = 0.5 * dot(grad(u), grad(u)) * dx - f * u * dx
        assert E.rank == 0
        R = derivative(E, u)
        assert R.rank == 1 and sorted(R.arguments()) == [0]
        assert R.arguments()[0] is V
        ref = bref.vector(inner(grad(u), grad(v)) * dx - f * v * dx)
        got = bref.vector(R)
        assert numpy.abs(got - ref).max() <= 1e-14 * numpy.abs(ref).max()
        H = derivative(R, u)
        assert H.rank == 2 and sorted(H.arguments()) == [0, 1]
        # (the load -f*u*dx does not depend on u any more: the part vanished)
        assert len(H.terms()) == 1
        K = bref.matrix(inner(grad(du), grad(v)) * dx).toarray()
        assert numpy.abs(bref.matrix(H).toarray() - K).max() \
            <= 1e-14 * numpy.abs(K).max()
        _same_tables(H.terms()[0][1], inner(grad(du), grad(v)) * dx)
        # the direction given explicitly
        _same_tables(derivative(E, u, v).terms()[0][1], R.terms()[0][1])
        _same_tables(derivative(R, u, du).terms()[0][1], H.terms()[0][1])


def test_parts_keep_sign_measure_and_degree():
    mesh, V1, V2 = _spaces()
    u = nref.state(V2)
    v = TestFunction(V2)
    k = fem.Constant(2.0)
    F = u**2 * v * dx - fem.exp(u) * v * dx(degree=3) \
        + k * v * dx + 2.0 * u * v.dx(0) * dx(mesh)
    J = derivative(F, u)
    assert isinstance(J, forms.FormSum)
    parts = J.terms()
    # (the part without u is gone; the others keep order and sign)
    assert [s for s, _ in parts] == [1.0, -1.0, 1.0]
    origin = [p for _, p in F.terms()]
    assert [p.derived_from for _, p in parts] == [origin[0], origin[1],
                                                   origin[3]]
    # the degree of the part it came from, or the metadata's
    assert [p.degree() for _, p in parts] == [6, 3, 3]
    assert parts[1][1].metadata == {'quadrature_degree': 3}
    assert parts[1][1].integrand.deg == origin[1].integrand.deg
    assert all(p.integral_type == 'cell' and p.mesh is mesh
               for _, p in parts)
    # a single form gives a single form
    single = derivative(u**2 * v * dx, u)
    assert type(single) is forms.Form and single.rank == 2


def test_equations():
    mesh, V1, V2 = _spaces()
    u = nref.state(V1)
    v = TestFunction(V1)
    F = u**2 * v * dx
    for zero in (0, 0.0, numpy.float64(0.0)):
        eq = F == zero
        assert isinstance(eq, forms.Equation)
        assert eq.lhs is F and eq.rhs == 0
        assert bool(eq) is False
        eq = (F - v * dx) == zero
        assert isinstance(eq, forms.Equation) and eq.rhs == 0
    for other in (1, -2.5):
        with pytest.raises(ValueError, match='== 0'):
            F == other
        with pytest.raises(ValueError, match='== 0'):
            (F + F) == other
    # what was there stays: a == L, identity for functionals, hashing
    du = TrialFunction(V1)
    a, L = du * v * dx, v * dx
    eq = a == L
    assert eq.lhs is a and eq.rhs is L
    m0 = fem.Constant(1.0) * dx(mesh)
    assert (m0 == m0) is True and (m0 == fem.Constant(1.0) * dx(mesh)) is False
    assert (F == 'zero') is False and (F == True) is False    # noqa: E712
    assert len({F, a, L, F}) == 3


def test_refusals():
    mesh, V1, V2 = _spaces()
    W = fem.VectorFunctionSpace(mesh, 'CG', 2)
    u, u2 = nref.state(V1), nref.state(V2)
    v, du = TestFunction(V1), TrialFunction(V1)
    F = u**2 * v * dx
    # rank 2: the result would be a rank-3 form, as in UFL
    with pytest.raises(NotImplementedError, match='derivative.*rank-3 form'):
        derivative(u * du * v * dx, u)
    with pytest.raises(NotImplementedError, match='derivative.*rank-3 form'):
        derivative(F + du * v * dx, u)
    # u on a vector space
    w = fem.Function(W)
    with pytest.raises(NotImplementedError, match='derivative.*vector'):
        derivative(dot(w, w) * v * dx, w)
    # (a Function never lives on a component view or a mixed space: Function
    # itself refuses those)
    # u does not occur
    with pytest.raises(ValueError, match='does not depend on u'):
        derivative(F, fem.Function(V1))
    with pytest.raises(ValueError, match='does not depend on u'):
        derivative(fem.Constant(1.0) * v * dx + v.dx(0) * dx, u)
    # u of another degree or mesh than the form's arguments
    with pytest.raises(ValueError, match='different spaces'):
        derivative(u2**2 * v * dx, u2)
    other = fem.FunctionSpace(fem.UnitSquareMesh(2, 2), 'CG', 1)
    with pytest.raises(ValueError, match='different spaces'):
        derivative(F, fem.Function(other))
    # the direction: only the argument with the right number, of u's space
    for bad in (du, TestFunction(V2), u, 1.0, v.dx(0), 2.0 * v):
        with pytest.raises(ValueError, match='du must be'):
            derivative(u**2 * dx, u, bad)
    with pytest.raises(ValueError, match='du must be'):
        derivative(F, u, v)
    # a functional over ds: the argument would land under ds
    with pytest.raises(NotImplementedError, match='contribution map'):
        derivative(u**2 * ds, u)
    with pytest.raises(NotImplementedError, match='contribution map'):
        derivative(u**2 * dx + u * ds(mesh), u)
    # ... unless that part does not hold u
    n = fem.FacetNormal(mesh)
    E = u**2 * dx + dot(fem.as_vector([1.0, 0.0]), n) * ds(mesh)
    assert derivative(E, u).rank == 1
    with pytest.raises(TypeError):
        derivative(u**2, u)
    with pytest.raises(TypeError):
        derivative(F, fem.Constant(1.0))
    # still stubs
    for name in ('action', 'adjoint'):
        with pytest.raises(NotImplementedError, match=name):
            getattr(fem, name)(F, u)
    assert fem.derivative is forms.derivative


def test_solve_parameters_and_refusals(monkeypatch):
    from flow_amd.fem import ops
    mesh, V1, V2 = _spaces()
    u = nref.state(V1)
    v, du = TestFunction(V1), TrialFunction(V1)
    F = (1 + u**2) * inner(grad(u), grad(v)) * dx - v * dx
    ns, symmetric = ops.newton_parameters(None)
    assert symmetric is False
    assert (ns['maximum_iterations'], ns['relative_tolerance'],
            ns['absolute_tolerance'], ns['relaxation_parameter'],
            ns['error_on_nonconvergence'], ns['convergence_criterion']) == (
                50, 1e-9, 1e-10, 1.0, True, 'residual')
    ns, symmetric = ops.newton_parameters({
        'nonlinear_solver': 'newton', 'symmetric': True,
        'newton_solver': {'maximum_iterations': 7, 'report': True,
                          'linear_solver': 'bicgstab',
                          'krylov_solver': {'relative_tolerance': 1e-8}}})
    assert symmetric and ns['maximum_iterations'] == 7 and ns['report']
    assert ns['krylov_solver'] == {'relative_tolerance': 1e-8}
    assert ns['relative_tolerance'] == 1e-9

    def solve(prm=None, F=F, u=u, **kw):
        return fem.solve(F == 0, u, solver_parameters=prm, **kw)

    with pytest.raises(ValueError, match='snes'):
        solve({'nonlinear_solver': 'snes'})
    with pytest.raises(ValueError, match='incremental'):
        solve({'newton_solver': {'convergence_criterion': 'incremental'}})
    with pytest.raises(ValueError, match='unknown keys.*line_search'):
        solve({'newton_solver': {'line_search': 'bt'}})
    with pytest.raises(ValueError, match='unknown keys.*snes_solver'):
        solve({'snes_solver': {}})
    with pytest.raises(ValueError, match='no direct solver'):
        solve({'newton_solver': {'linear_solver': 'lu'}})
    # F: rank 1 in the test function of u's space, holding u
    with pytest.raises(ValueError, match='rank 1'):
        solve(F=u**2 * dx)
    with pytest.raises(ValueError, match='rank 1'):
        solve(F=du * v * dx)
    with pytest.raises(ValueError, match='space of the test'):
        solve(u=nref.state(V2))
    with pytest.raises(ValueError, match='does not depend on u'):
        solve(u=fem.Function(V1))
    # J: rank 2 on V
    for bad in (F, u**2 * dx, TrialFunction(V2) * TestFunction(V2) * dx, 1.0):
        with pytest.raises(ValueError, match='J must be a bilinear'):
            solve(J=bad)
    # J= belongs to the nonlinear solve
    with pytest.raises(ValueError, match='J='):
        fem.solve(du * v * dx == v * dx, u, J=du * v * dx)
    # the jobs of one assembly: what fuses, what goes through the pair
    J = derivative(F, u)
    jobs = ops.newton_jobs(J, F)
    assert [j[0] for j in jobs] == ['newton', 'vector']
    assert jobs[0][3].nout == forms.NEWTON_SLOTS and jobs[0][4:6] == (
        2, 'default')       # (P1: degree 2 of 1 + u^2, the gradients 0)
    # (the record of a scalar job: no ds part, tag 0, the fused pair of parts)
    assert jobs[0].part is None and jobs[0].tag == 0
    assert jobs[0].call == (0, 0) and jobs[1].call == (None, 1)
    assert [j[0] for j in ops.newton_jobs(J, F, fuse=False)] == [
        'matrix', 'vector', 'vector']
    # another degree on the residual's part: no partner, the pair
    G = (1 + u**2) * inner(grad(u), grad(v)) * dx(degree=3)
    assert [j[0] for j in ops.newton_jobs(derivative(F, u), G)] == [
        'matrix', 'vector']
    # not on strips
    from flow_amd import parallel
    monkeypatch.setattr(parallel, 'active', lambda: True)
    with pytest.raises(NotImplementedError, match='on strips'):
        solve()
    assert issubclass(_hip.NotConverged, RuntimeError)


def _quasilinear_tables(V):
    u = nref.state(V)
    v = TestFunction(V)
    F = (1 + u**2) * inner(grad(u), grad(v)) * dx
    J = derivative(F, u)
    return u, J.argument_table()[1], F.argument_table()[1]


def test_newton_program_shares_subtrees():
    mesh, V1, V2 = _spaces()
    u, tJ, tF = _quasilinear_tables(V2)
    plain = forms.newton_program(tJ, tF, share=False)
    shared = forms.newton_program(tJ, tF)
    print('quasilinear: %d instructions without sharing, %d with'
          % (len(plain.code), len(shared.code)))
    assert len(shared.code) < len(plain.code)
    assert plain.nout == shared.nout == 12
    # slots 3 b + a of the Jacobian and 9 + b of the residual
    assert shared.slots == plain.slots == [3, 4, 6, 8, 10, 11]
    # without sharing: the two programs of the pair, one after the other
    pj, pf = forms.argument_program(tJ, 2), forms.argument_program(tF, 1)
    # (operation and destination; the operand tables are merged)
    assert [ins[:2] for ins in plain.code] == [
        ins[:2] for ins in pj.code + pf.code]
    leaves = nref.Leaves(40, seed=1)
    want = {3 * b + a: nref.eval_tree(tJ[b][a], leaves) for b in range(3)
            for a in range(3) if tJ[b][a] is not None}
    want.update({9 + b: nref.eval_tree(tF[b], leaves) for b in range(3)
                 if tF[b] is not None})
    for prog in (plain, shared):
        got = nref.run_program(prog, leaves)
        assert sorted(got) == sorted(want) == prog.slots
        for k in want:
            assert numpy.array_equal(got[k], want[k]), k
    # the shared registers come from the top and are written once
    mov = forms.OPS['mov']
    tops = [ins[1] for ins in shared.code if ins[0] == mov and ins[1] >= 4]
    assert tops and len(set(tops)) == len(tops)
    assert max(tops) == forms.REGISTERS - 1
    # the residuals of the other tests: the same 12 values either way
    u = nref.state(V2)
    for name, F in nref.residuals(mesh, V2, u):
        part = F.terms()[0][1]
        tF = part.argument_table()[1]
        tJ = derivative(part, u).argument_table()[1]
        try:
            shared = forms.newton_program(tJ, tF)
        except ValueError as e:
            print('%-28s does not fit: %s' % (name, e))
            continue
        want = nref.run_program(forms.argument_program(tJ, 2), leaves)
        want = {k: x for k, x in want.items()}
        want.update({9 + k: x for k, x in nref.run_program(
            forms.argument_program(tF, 1), leaves).items()})
        got = nref.run_program(shared, leaves)
        n0 = len(forms.argument_program(tJ, 2).code) \
            + len(forms.argument_program(tF, 1).code)
        print('%-28s %d -> %d instructions, %d registers'
              % (name, n0, len(shared.code), shared.nregs))
        assert len(shared.code) <= n0
        assert sorted(got) == sorted(want)
        for k in want:
            assert numpy.array_equal(got[k], want[k]), (name, k)


def test_programs_without_sharing_are_unchanged():
    # 'reg' leaves and the shared list are newton_program's alone
    mesh, V1, V2 = _spaces()
    u, tJ, tF = _quasilinear_tables(V1)
    prog = forms.argument_program(tJ, 2)
    assert prog.nout == 9
    assert all(ins[0] != forms.OPS['mov'] for ins in prog.code)
    # a program over the limits is a ValueError: the caller's fallback
    t = ('field', u, 0, 0)
    big = t
    for i in range(16):
        big = ('add', ('mul', big, ('num', float(i + 2))), ('sin', t))
    table = [[None] * 3 for _ in range(3)]
    table[0][0] = big
    with pytest.raises(ValueError, match='instructions'):
        forms.newton_program(table, [big, None, None], share=False)


def test_newton_on_the_host_converges_quadratically():
    '''-div((1 + u^2) grad u) = f, u_exact = sin(pi x) sin(pi y), n = 8, from
    u = 0, with the evaluator's J = derivative(F, u) and a sparse LU.  An
    exact Jacobian gives r_(k+1) <= C r_k^2; an inexact one converges
    linearly, r_(k+1) = c r_k, and then r_(k+1) / r_k^2 = c / r_k passes any
    bound as r_k falls (10 once r_k < c / 10; the residuals reach 1e-6).
    Measured ratios, P1: 0.57 0.11 0.12 0.11 0.071; P2: 1.13 0.17 0.20 0.16
    0.15 (5 iterations each).'''
    for degree in (1, 2):
        V, u, F, bcs, exact = nref.quasilinear_problem(8, degree)
        res, its = nref.host_newton(F, u, bcs)
        ratios = [res[i + 1] / res[i]**2 for i in range(len(res) - 1)]
        print('P%d: %d iterations, residuals %s, ratios %s'
              % (degree, its, res, ratios))
        assert res[-1] < 1e-9 * res[0] and len(ratios) >= 4
        assert max(ratios[-3:]) < 10.0
        err = fem.errornorm(exact, u)
        print('P%d L2 error %.3e' % (degree, err))
        assert err < (3e-2 if degree == 1 else 2e-3)


def test_overlong_tables_split_into_programs():
    '''The Jacobian of the minimal-surface residual does not fit one program
    (152 instructions): argument_programs deals its slots to two, each
    written once, with the values of the table; tables that fit stay the one
    program of argument_program.'''
    mesh, V1, V2 = _spaces()
    u = nref.state(V2)
    names = dict(nref.residuals(mesh, V2, u))
    F = names['minimal surface']
    tJ = derivative(F, u).argument_table()[1]
    with pytest.raises(ValueError, match='instructions'):
        forms.argument_program(tJ, 2)
    progs = forms.argument_programs(tJ, 2)
    print([(len(p.code), p.slots) for p in progs])
    assert len(progs) == 2 and all(p.nout == 9 for p in progs)
    leaves = nref.Leaves(30, seed=2)
    got = {}
    for p in progs:
        out = nref.run_program(p, leaves)
        assert not set(out) & set(got)
        got.update(out)
    want = {3 * b + a: nref.eval_tree(tJ[b][a], leaves) for b in range(3)
            for a in range(3) if tJ[b][a] is not None}
    assert sorted(got) == sorted(want) == [4, 5, 7, 8]
    for k in want:
        assert numpy.array_equal(got[k], want[k]), k
    # its jobs: two matrix programs and the residual's vector
    assert [j[0] for j in fem.ops.newton_jobs(derivative(F, u), F)] == [
        'matrix', 'matrix', 'vector']
    # a table that fits: the program of argument_program, unchanged
    tq = derivative(names['quasilinear'], u).argument_table()[1]
    one = forms.argument_programs(tq, 2)
    assert len(one) == 1 and one[0].code == forms.argument_program(tq, 2).code
