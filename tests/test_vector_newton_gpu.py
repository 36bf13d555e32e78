# -*- coding: utf-8 -*-
'''
derivative() and solve(F == 0) on vector spaces on the HIP path
(flow_form_block_newton): the fused block Newton assembly against the pair
flow_form_block_matrix / flow_form_block_vector, bit for bit, and against
the numpy evaluator; the fallback for tables that do not fit a fused program
(St. Venant-Kirchhoff); Newton's method against the host Newton, its orders,
its quadratic convergence, the two linear-solver routes and the parameters.
'''
import numpy
import pytest

from flow_amd import fem, _hip
from flow_amd.fem import ops
from flow_amd.fem import (
    TestFunction, TrialFunction, assemble, derivative, dx, dot, inner, grad,
    )

import vector_form_reference as vref
import vector_newton_reference as vnref

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _switches_on():
    with fem.vector_arguments(True), fem.facet_arguments(True), \
            fem.vector_derivatives(True):
        yield


MESHES = {'square': lambda: fem.UnitSquareMesh(12, 9),
          'karman': lambda: fem.karman_channel(60, 14, fitted=True)}


def _err(got, ref, what=''):
    '''max entrywise error relative to max|entry| (printed: the measured
    figure is part of the record).'''
    got = got.toarray() if hasattr(got, 'toarray') else numpy.asarray(got)
    ref = ref.toarray() if hasattr(ref, 'toarray') else numpy.asarray(ref)
    e = numpy.abs(got - ref).max() / numpy.abs(ref).max()
    print('%-56s %.2e' % (what, e))
    return e


def _planes(A):
    return [A.plane(p).cpu().numpy().copy() for p in range(4)]


def _diagonal(W, u):
    '''A residual whose Jacobian has no off-diagonal block.'''
    v = TestFunction(W)
    F = (inner(grad(u), grad(v)) + u[0]**3 * v[0] + u[1]**3 * v[1]) * dx
    return F, None


def _check_assembly(name, W, u, F, host):
    tag = '%s P%d ' % (name, W.degree)
    J = derivative(F, u)
    fused = ops.NewtonAssembler(J, F, W)
    pair = ops.NewtonAssembler(J, F, W, fuse=False)
    assert not pair.fused
    assert not any(j[0] == 'newton' for j in pair.jobs)
    if name == 'kirchhoff':
        # no fused program fits: the request falls back to the pair
        assert not fused.fused
        assert set(j[0] for j in fused.jobs) == {'matrix', 'vector'}
    else:
        assert fused.fused
        assert [j[0] for j in fused.jobs].count('newton') == 2
    A0, b0 = assemble(J), assemble(F)
    assert A0.kind == 2
    ref = _planes(A0) + [b0.get_local().copy()]
    for label, asm in (('fused', fused), ('pair', pair)):
        for call in range(2):
            A, b = asm.assemble()
            assert A.kind == 2 and b.numel() == W.size()
            got = _planes(A) + [b.cpu().numpy().copy()]
            for k in range(5):
                assert numpy.array_equal(got[k], ref[k]), (tag, label, call, k)
    A, b = fused.assemble()
    if name == 'diagonal':
        planes = _planes(A)
        assert not planes[1].any() and not planes[2].any()
        assert planes[0].any() and planes[3].any()
    if host:
        assert _err(A.to_scipy(), vref.matrix(J), tag + 'J vs host') < 1e-12
        assert _err(b.cpu().numpy(), vref.vector(F), tag + 'F vs host') < 1e-12
    # another state: the structs follow the field, the buffers stay
    u.set_array(0.5 * u.array())
    A, b = fused.assemble()
    A1, b1 = assemble(J), assemble(F)
    for p in range(4):
        assert numpy.array_equal(A.plane(p).cpu().numpy(),
                                 A1.plane(p).cpu().numpy())
    assert numpy.array_equal(b.cpu().numpy(), b1.get_local())


CASES = {'burgers': (vnref.burgers, vnref.state),
         'forchheimer': (vnref.forchheimer, vnref.state),
         'traction robin': (vnref.traction_robin, vnref.state),
         'diagonal': (_diagonal, vnref.state),
         'kirchhoff': (vnref.kirchhoff, vnref.small_state)}


@pytest.mark.parametrize('degree', (1, 2))
@pytest.mark.parametrize('mesh_name', sorted(MESHES))
def test_fused_against_pair_and_host(hip, mesh_name, degree):
    '''NewtonAssembler(fuse=True) against fuse=False and both against
    assemble(J) / assemble(F): the same bits in all four planes and in the 2N
    vector, on a second call too; absent blocks exactly zero; both against the
    host evaluator below 1e-12 relative to max|entry|.'''
    mesh = MESHES[mesh_name]()
    W = fem.VectorFunctionSpace(mesh, 'CG', degree)
    for name in ('burgers', 'forchheimer', 'traction robin', 'diagonal'):
        make, state = CASES[name]
        u = state(W)
        _check_assembly(name, W, u, make(W, u)[0], host=True)


@pytest.mark.parametrize('degree', (1, 2))
def test_kirchhoff_fallback(hip, degree):
    '''St. Venant-Kirchhoff: 12 programs for J, 4 for F, none of the combined
    ones fits -- the pair's launches, the same bits, the host's values.'''
    W = fem.VectorFunctionSpace(MESHES['square'](), 'CG', degree)
    u = vnref.small_state(W)
    _check_assembly('kirchhoff', W, u, vnref.kirchhoff(W, u)[0], host=True)
    W = fem.VectorFunctionSpace(MESHES['karman'](), 'CG', degree)
    u = vnref.small_state(W)
    _check_assembly('kirchhoff', W, u, vnref.kirchhoff(W, u)[0], host=False)


def _rel(u, ur):
    return numpy.linalg.norm(u.array() - ur.array()) \
        / numpy.linalg.norm(ur.array())


def test_burgers_solve_orders_and_convergence(hip):
    '''Viscous Burgers with a manufactured solution and Dirichlet data on W,
    from u = 0.  At n = 8: the iteration count of the host Newton and its
    solution to 1e-7 relative l2 (the bound of the scalar Newton test), and
    quadratic convergence: the last two ratios r[k+1] / r[k]^2 stay below C =
    10 x the largest such ratio of the host Newton's own residuals.  L2
    orders over n = 8, 16, 32 within 0.1 of 2 (P1) and 3 (P2).'''
    for degree, order in ((1, 1.9), (2, 2.9)):
        errs = []
        for n in (8, 16, 32):
            W, u, F, bcs, exact = vnref.burgers_problem(n, degree)
            info = fem.solve(F == 0, u, bcs)
            assert info.converged and info.fused
            assert info.method == 'gmres+ilu0'
            assert len(info.residuals) == info.iterations + 1
            assert len(info.linear_iterations) == info.iterations
            errs.append(fem.errornorm(exact, u))
            if n == 8:
                Wr, ur, Fr, bcr, _ = vnref.burgers_problem(n, degree)
                res, its = vnref.host_newton(Fr, ur, bcr)
                print('P%d residuals, device: %s' % (degree, info.residuals))
                print('P%d residuals, host:   %s' % (degree, res))
                assert info.iterations == its
                e = _rel(u, ur)
                print('P%d n = 8: %r; rel l2 vs host Newton %.2e'
                      % (degree, info, e))
                assert e < 1e-7
                C = 10.0 * max(res[k + 1] / res[k]**2
                               for k in (len(res) - 3, len(res) - 2))
                r = info.residuals
                for k in (len(r) - 3, len(r) - 2):
                    print('P%d r[%d] / r[%d]^2 = %.3e (C = %.3e)'
                          % (degree, k + 1, k, r[k + 1] / r[k]**2, C))
                    assert r[k + 1] <= C * r[k]**2
        rates = numpy.log2(numpy.array(errs[:-1]) / numpy.array(errs[1:]))
        print('P%d errors %s orders %s' % (degree, errs, rates))
        assert (rates > order).all()


def _forchheimer_problem(degree):
    W = fem.VectorFunctionSpace(fem.UnitSquareMesh(8, 8), 'CG', degree)
    u = fem.Function(W)
    F, _ = vnref.forchheimer(W, u)
    bcs = [fem.DirichletBC(W.sub(0), fem.Expression('0.2*x[1]', degree=1),
                           'on_boundary')]
    return W, u, F, bcs


def test_forchheimer_solve(hip):
    '''Forchheimer-Brinkman with a condition on W.sub(0) only, from a state
    away from u = 0 (the drag is not differentiable there up to the 1e-8):
    the non-symmetric route, fused, against the host Newton.'''
    for degree in (1, 2):
        W, u, F, bcs = _forchheimer_problem(degree)
        Wr, ur, Fr, bcr = _forchheimer_problem(degree)
        for w in (u, ur):
            w.set_array(vnref.state(W).array())
        info = fem.solve(F == 0, u, bcs)
        res, its = vnref.host_newton(Fr, ur, bcr)
        e = _rel(u, ur)
        print('Forchheimer P%d: %r (host: %d iterations, %s); rel l2 %.2e'
              % (degree, info, its, res, e))
        assert info.converged and info.fused
        # ('gmres' with its preconditioner's suffix, as the scalar solve
        # reports it)
        assert info.method.split('+')[0] == 'gmres'
        assert info.method == 'gmres+ilu0'
        assert info.iterations == its
        assert e < 1e-7


def _robin_problem(degree):
    W = fem.VectorFunctionSpace(fem.UnitSquareMesh(8, 8), 'CG', degree)
    u = fem.Function(W)
    F, _ = vnref.traction_robin(W, u)
    bcs = [fem.DirichletBC(W, fem.Constant((0.5, -0.25)), vnref.Side(
        lambda x: x[1] < 1e-12))]
    return W, u, F, bcs


def test_traction_robin_solve(hip):
    for degree in (1, 2):
        W, u, F, bcs = _robin_problem(degree)
        Wr, ur, Fr, bcr = _robin_problem(degree)
        info = fem.solve(F == 0, u, bcs)
        res, its = vnref.host_newton(Fr, ur, bcr)
        e = _rel(u, ur)
        print('traction / Robin P%d: %r (host: %d iterations); rel l2 %.2e'
              % (degree, info, its, e))
        assert info.converged and info.fused and info.iterations == its
        assert e < 1e-7


def _burgers(**kw):
    W, u, F, bcs, _ = vnref.burgers_problem(8, 2)
    return fem.solve(F == 0, u, bcs, **kw), u, F, bcs


def test_routes_and_parameters(hip):
    # a residual whose Jacobian is block-symmetric: CG + Jacobi
    W = fem.VectorFunctionSpace(fem.UnitSquareMesh(8, 8), 'CG', 2)
    v, du = TestFunction(W), TrialFunction(W)
    f = fem.Expression(vnref.SOURCE, degree=2)
    bcs = [fem.DirichletBC(W, fem.Constant((0.1, 0.2)), 'on_boundary')]
    us, ur = fem.Function(W), fem.Function(W)
    info = fem.solve(_diagonal(W, us)[0] - dot(f, v) * dx == 0, us, bcs)
    res, its = vnref.host_newton(_diagonal(W, ur)[0] - dot(f, v) * dx, ur, bcs)
    print('symmetric: %r; rel l2 vs host Newton %.2e' % (info, _rel(us, ur)))
    assert info.converged and info.method == 'cg'
    assert _rel(us, ur) < 1e-7
    # a linear F: one iteration, the solution of solve(a == L)
    ul, un = fem.Function(W), fem.Function(W)
    fem.solve((inner(grad(du), grad(v)) + dot(du, v)) * dx == dot(f, v) * dx,
              ul, bcs)
    info = fem.solve((inner(grad(un), grad(v)) + dot(un, v) - dot(f, v)) * dx
                     == 0, un, bcs)
    print('linear F: %r; rel l2 vs solve(a == L) %.2e' % (info, _rel(un, ul)))
    assert info.converged and info.iterations == 1 and info.method == 'cg'
    assert _rel(un, ul) < 1e-10
    # damping: slower, the same solution
    full, u1, _, _ = _burgers()
    half, u2, _, _ = _burgers(solver_parameters={
        'newton_solver': {'relaxation_parameter': 0.5}})
    print('relaxation 1.0: %d iterations, 0.5: %d' % (full.iterations,
                                                     half.iterations))
    assert half.converged and half.iterations > full.iterations
    assert _rel(u2, u1) < 1e-7
    # one iteration is not enough
    with pytest.raises(_hip.NotConverged):
        _burgers(solver_parameters={'newton_solver': {'maximum_iterations': 1}})
    info, _, _, _ = _burgers(solver_parameters={'newton_solver': {
        'maximum_iterations': 1, 'error_on_nonconvergence': False}})
    assert info.converged is False and info.iterations == 1
    assert len(info.residuals) == 2
    # J= the default, given: the same bits
    W3, u3, F3, bcs3, _ = vnref.burgers_problem(8, 2)
    info3 = fem.solve(F3 == 0, u3, bcs3, J=derivative(F3, u3))
    assert info3.fused and info3.residuals == full.residuals
    assert numpy.array_equal(u3.array(), u1.array())
