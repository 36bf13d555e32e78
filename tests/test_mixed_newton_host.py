# -*- coding: utf-8 -*-
'''
Host logic of Newton's method on a Taylor-Hood space (fem.mixed_derivatives;
flow_amd/fem/forms.py, function.py, mixed.py): the views of a mixed Function
know their owner, derivative() with respect to it gives the leaves of
TrialFunctions, the blocks of the Navier-Stokes Jacobian against the
hand-written Newton form, which blocks are frozen, the errors with the switch
off (unchanged) and the refusals with it on.  No GPU.
'''
import pytest

from flow_amd import fem, _hip
from flow_amd.fem import (
    TestFunctions, TrialFunctions, dx, dS, dot, inner, grad, div, solve,
    derivative,
    )
from flow_amd.fem import forms, mixed


@pytest.fixture(autouse=True)
def _switches_on():
    with fem.mixed_arguments(True), fem.vector_arguments(True):
        yield


def _space(mesh, kv=2, kp=1):
    return fem.FunctionSpace(
        mesh, fem.VectorElement('Lagrange', 'triangle', kv)
        * fem.FiniteElement('Lagrange', 'triangle', kp))


def _navier_stokes(WP, w):
    (u, p) = fem.split(w)
    (v, q) = TestFunctions(WP)
    nu = fem.Constant(0.05)
    f = fem.Constant((0.3, -0.1))
    return nu * inner(grad(u), grad(v)) * dx + dot(dot(grad(u), u), v) * dx \
        - p * div(v) * dx - q * div(u) * dx - inner(f, v) * dx, nu, u, p


def _merged(form):
    '''{(block r, block s, b, a): coefficient tree} of a rank-2 mixed form,
    the signed parts added with the module's own folding.'''
    out = {}
    for sign, part in form.terms():
        rank, table = part.argument_table()
        assert rank == 2 and isinstance(table, forms.MixedTable)
        for r in range(3):
            for s in range(3):
                if table[r][s] is None:
                    continue
                for b in range(3):
                    for a in range(3):
                        c = table[r][s][b][a]
                        if c is None:
                            continue
                        c = c if sign == 1.0 else forms.s_neg(c)
                        key = (r, s, b, a)
                        out[key] = forms.s_add(out[key], c) if key in out \
                            else c
    return out


def test_switch():
    assert issubclass(fem.mixed_derivatives, forms._Switch)
    assert fem.mixed_derivatives is forms.mixed_derivatives
    assert fem.mixed_derivatives.enabled is False
    with fem.mixed_arguments(False), fem.vector_arguments(False):
        with fem.mixed_derivatives(True) as sw:
            assert sw.previous is False and fem.mixed_derivatives.enabled
            # it implies no other switch
            assert not forms.mixed_arguments.enabled
            assert not forms.vector_arguments.enabled
            assert not forms.mixed_gmres.enabled
            assert not forms.facet_arguments.enabled
    assert fem.mixed_derivatives.enabled is False


def test_views_know_their_owner():
    WP = _space(fem.UnitSquareMesh(3, 2))
    w, other = fem.Function(WP), fem.Function(WP)
    for views in (w.split(), fem.split(w), (w.sub(0), w.sub(1))):
        for i, view in enumerate(views):
            assert view.mixed_owner[0] is w and view.mixed_owner[1] == i
    (u1, p1), (u2, p2) = fem.split(w), fem.split(w)
    assert u1 is not u2 and p1 is not p2
    for a, b in ((u1, u2), (p1, p2)):
        assert a.mixed_owner == b.mixed_owner
        assert a.mixed_owner[0] is b.mixed_owner[0]
    # a deep copy is a field of its own; so are w itself and plain Functions
    for copy in w.split(deepcopy=True):
        assert copy.mixed_owner is None
    assert w.mixed_owner is None
    assert fem.Function(WP.sub(1)).mixed_owner is None
    assert fem.split(other)[0].mixed_owner[0] is other
    # what a view was before: a Function on the sub-space over w's storage
    assert u1.function_space().same_as(WP.sub(0))
    assert u1.data.data_ptr() == w.data.data_ptr()


def test_depends_on_sees_through_views():
    WP = _space(fem.UnitSquareMesh(3, 2))
    w, other = fem.Function(WP), fem.Function(WP)
    (u, p) = fem.split(w)
    (v, q) = TestFunctions(WP)
    tree = (dot(u, v) * dx).integrand.comps
    assert forms.depends_on(tree, w)
    assert not forms.depends_on(tree, other)
    assert forms.depends_on((p * q * dx).integrand.comps, w)
    uc, pc = w.split(deepcopy=True)
    assert not forms.depends_on((dot(uc, v) * dx + pc * q * dx).terms()[0][1]
                                .integrand.comps, w)
    # a Function is still recognised as itself
    V = fem.FunctionSpace(fem.UnitSquareMesh(3, 2), 'Lagrange', 1)
    g = fem.Function(V)
    assert forms.depends_on((g * g * dx).integrand.comps, g)
    assert not forms.depends_on((g * g * dx).integrand.comps, fem.Function(V))


def test_derivative_gives_the_leaves_of_trial_functions():
    WP = _space(fem.UnitSquareMesh(3, 2))
    w, other = fem.Function(WP), fem.Function(WP)
    (u, p) = fem.split(w)
    (v, q) = TestFunctions(WP)
    (du, dp) = TrialFunctions(WP)
    with fem.mixed_derivatives(True):
        J = derivative(u[1] * v[0] * dx + p * q * dx, w)
        assert J.rank == 2
        (_, a), (_, b) = J.terms()
        assert a.integrand.comps == (du[1] * v[0]).comps
        assert b.integrand.comps == (dp * q).comps
        # the derived part keeps degree, measure and subdomain of its parent
        part = p * p * q * dx(degree=5)
        Jp = derivative(part, w)
        assert Jp.integral_type == part.integral_type
        assert Jp.integrand.deg == part.integrand.deg
        assert Jp.metadata == part.metadata
        assert Jp.derived_from is part
        # rank 0: the new argument is the test function
        G = derivative(0.5 * dot(u, u) * dx + p * dx, w)
        assert G.rank == 1
        assert set(G.arguments()) == {0}
        assert derivative(0.5 * dot(u, u) * dx, w, TestFunctions(WP)).rank == 1
        # du given: the pair of TrialFunctions(WP)
        assert derivative(p * q * dx, w, (du, dp)).integrand.comps \
            == (dp * q).comps
        # views of two calls of split are one field: both factors count
        u2, p2 = fem.split(w)
        Jt = derivative(p * p2 * q * dx, w)
        assert Jt.integrand.comps == ((dp * p2 + p * dp) * q).comps
        # a deep copy and a view of another Function are coefficients
        uc, pc = w.split(deepcopy=True)
        uo, po = fem.split(other)
        with pytest.raises(ValueError, match='does not depend on u'):
            derivative(dot(uc, v) * dx + pc * q * dx + po * q * dx, w)
        Jm = derivative(dot(uo, u) * q * dx, w)
        assert not forms.depends_on(Jm.integrand.comps, w)
        assert forms.depends_on(Jm.integrand.comps, other)


def test_navier_stokes_jacobian_is_the_hand_written_newton_form():
    WP = _space(fem.UnitSquareMesh(3, 2))
    w = fem.Function(WP)
    F, nu, u, p = _navier_stokes(WP, w)
    (v, q) = TestFunctions(WP)
    (du, dp) = TrialFunctions(WP)
    with fem.mixed_derivatives(True):
        J = derivative(F, w)
    hand = (nu * inner(grad(du), grad(v)) + dot(dot(grad(du), u), v)
            + dot(dot(grad(u), du), v) - dp * div(v) - q * div(du)) * dx
    # the source term drops out; every part's table is a MixedTable
    assert J.rank == 2 and len(J.terms()) == 4
    for _, part in J.terms():
        assert isinstance(part.argument_table()[1], forms.MixedTable)
    got, want = _merged(J), _merged(hand)
    blocks = lambda t: sorted(set(k[:2] for k in t))    # noqa: E731
    assert blocks(got) == blocks(want) == [
        (0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (1, 2), (2, 0), (2, 1)]
    assert sorted(got) == sorted(want)
    for key in want:
        assert got[key] == want[key], key
    # written part by part as derivative() leaves them, the tables are equal
    # part by part (tests/test_mixed_newton_gpu.py asks for equal bits then)
    parts = nu * inner(grad(du), grad(v)) * dx \
        + (dot(dot(grad(du), u), v) + dot(dot(grad(u), du), v)) * dx \
        - dp * div(v) * dx - q * div(du) * dx
    assert len(parts.terms()) == len(J.terms())
    for (s1, a), (s2, b) in zip(J.terms(), parts.terms()):
        assert s1 == s2
        assert a.argument_table() == b.argument_table()


def test_frozen_blocks():
    WP = _space(fem.UnitSquareMesh(3, 2))
    w = fem.Function(WP)
    F, nu, u, p = _navier_stokes(WP, w)
    (v, q) = TestFunctions(WP)
    with fem.mixed_derivatives(True):
        J = derivative(F, w)
        reads = mixed.block_dependence(J, WP, w)
        assert reads == {'uu': True, 'up0': False, 'up1': False,
                         'pu0': False, 'pu1': False}
        # without naming w: a view of any Function of WP
        assert mixed.block_dependence(J, WP) == reads
        assert mixed.block_dependence(J, WP, fem.Function(WP)) \
            == dict.fromkeys(reads, False)
        asm = mixed.MixedNewtonAssembler(J, F, WP, w=w)
        assert asm.frozen == ('up0', 'up1', 'pu0', 'pu1')
        assert asm.route == 'by_parts'
        # a coupling that reads w, and a constant pp block
        F2 = F - p * p * div(v) * dx - 1e-3 * p * q * dx
        asm = mixed.MixedNewtonAssembler(derivative(F2, w), F2, WP, w=w)
        assert asm.frozen == ('pp', 'pu0', 'pu1')
    assert fem.ops.NewtonInfo(False, 'cg').frozen == ()


def test_switch_off_keeps_the_errors():
    WP = _space(fem.UnitSquareMesh(3, 2))
    w = fem.Function(WP)
    F = _navier_stokes(WP, w)[0]
    assert not fem.mixed_derivatives.enabled
    with pytest.raises(NotImplementedError) as err:
        derivative(F, w)
    assert str(err.value) == (
        'derivative with respect to a Function of a vector, component or '
        'mixed space: only scalar P1 / P2 spaces carry arguments')
    with pytest.raises(NotImplementedError) as err:
        solve(F == 0, w, [])
    assert str(err.value) == (
        'solve(F == 0) on a mixed space: Newton\'s method takes scalar and '
        'vector spaces only')


def test_refusals_with_the_switch_on():
    mesh = fem.UnitSquareMesh(3, 2)
    WP, other = _space(mesh), _space(mesh, 1, 1)
    w = fem.Function(WP)
    F, nu, u, p = _navier_stokes(WP, w)
    (v, q) = TestFunctions(WP)
    (du, dp) = TrialFunctions(WP)
    with fem.mixed_derivatives(True):
        # a bad du
        for bad in (du, (dp, du), (v, q), TrialFunctions(other),
                    fem.TrialFunction(WP.sub(1)), (du, dp, dp)):
            with pytest.raises(ValueError, match='du must be the pair'):
                derivative(F, w, bad)
        with pytest.raises(ValueError, match='du must be the pair'):
            derivative(p * dx, w, (du, dp))
        # a dS part
        with fem.interior_facets(True):
            with pytest.raises(NotImplementedError, match='dS part'):
                derivative(F + fem.jump(p) * fem.jump(p) * dS(mesh), w)
            with fem.mixed_gmres(True):
                with pytest.raises(NotImplementedError, match='dS'):
                    solve(F + fem.avg(p) * fem.avg(q) * dS(mesh) == 0, w, [])
        # a ds part needs facet_arguments
        with pytest.raises(NotImplementedError, match='facet_arguments'):
            derivative(F + p * p * q * fem.ds(mesh), w)
        with fem.mixed_gmres(True):
            # J of another space
            (uo, po), (vo, qo) = TrialFunctions(other), TestFunctions(other)
            with pytest.raises(ValueError, match='J must be a bilinear form'):
                solve(F == 0, w, [], J=inner(grad(uo), grad(vo)) * dx
                      - po * div(vo) * dx)
            with pytest.raises(ValueError, match='J must be a bilinear form'):
                solve(F == 0, w, [], J=F)
            # 'two_level'
            with pytest.raises(ValueError, match="'ilu0' or 'jacobi'"):
                solve(F == 0, w, [], solver_parameters={
                    'newton_solver': {'preconditioner': 'two_level'}})
            # the rules of ops.newton_parameters hold
            with pytest.raises(ValueError, match='unknown keys'):
                solve(F == 0, w, [], solver_parameters={
                    'newton_solver': {'line_search': 'bt'}})
            # a form that does not read w
            with pytest.raises(ValueError, match='does not depend on w'):
                solve(inner(fem.Constant((1.0, 0.0)), v) * dx == 0, w, [])
        # mixed_gmres off: the error names the switch
        assert not fem.mixed_gmres.enabled
        with pytest.raises(NotImplementedError, match='mixed_gmres'):
            solve(F == 0, w, [])
