# -*- coding: utf-8 -*-
'''
derivative() and solve(F == 0) on the HIP path: the fused Jacobian-and-residual
pass (flow_form_newton) against the pair flow_form_matrix / flow_form_vector
and against the numpy evaluator, the silent fallback, and Newton's method
against the host Newton of tests/newton_reference.py (orders, iteration
counts, solutions), its parameters, and a heat-conduction example with a
temperature-dependent conductivity.  Meshes stay small.
'''
import numpy
import pytest

from flow_amd import fem, _hip, materials, message
from flow_amd.fem import (
    TestFunction, TrialFunction, assemble, dx, ds, dot, inner, grad, sin, exp,
    sqrt, derivative, ops,
    )

import bilinear_reference as bref
import newton_reference as nref

pytestmark = pytest.mark.gpu


def _meshes():
    return [fem.UnitSquareMesh(12, 9),
            fem.karman_channel(60, 14, fitted=True),
            fem.karman_channel_graded(lcar=1.0e-2)]


def _err(got, ref, what=''):
    got = got.toarray() if hasattr(got, 'toarray') else numpy.asarray(got)
    ref = ref.toarray() if hasattr(ref, 'toarray') else numpy.asarray(ref)
    e = numpy.abs(got - ref).max() / numpy.abs(ref).max()
    print('%-58s %.2e' % (what, e))
    return e


def _assembled(J, F, V, fuse):
    asm = ops.NewtonAssembler(J, F, V, fuse=fuse)
    A, b = asm.assemble()
    return asm, A.plane(0).cpu().numpy().copy(), b.cpu().numpy().copy(), A


def test_fused_against_pair_and_host(hip):
    '''flow_form_newton against flow_form_matrix + flow_form_vector and both
    against the numpy evaluator.  Fused against pair: the coefficient programs
    and the accumulation run the same instructions in the same order, so the
    results are asserted bit-identical (the issue's bound was 1e-12 relative
    to max|entry|).  Against the evaluator: entrywise relative to max|entry|,
    bound 1e-12, the project's bound; measured 1e-16 .. 2.8e-13.  The
    Jacobian of the minimal-surface residual exceeds one program (152
    instructions, 100 with its tables fused): it is assembled by the pair in
    two programs whose cell matrices add up (forms.argument_programs), so
    for it the fused request and the pair are the same launches.'''
    total = 0
    for m, mesh in enumerate(_meshes()):
        for k in (1, 2):
            V = fem.FunctionSpace(mesh, 'CG', k)
            u = nref.state(V)
            for name, F in nref.residuals(mesh, V, u):
                J = derivative(F, u)
                tag = 'mesh %d P%d %s: ' % (m, k, name)
                asm, vf, bf, Af = _assembled(J, F, V, True)
                if name == 'minimal surface':
                    assert [j[0] for j in asm.jobs] == ['matrix', 'matrix',
                                                        'vector']
                else:
                    assert asm.fused and asm.jobs[0][0] == 'newton'
                pair, vp, bp, Ap = _assembled(J, F, V, False)
                assert not pair.fused
                # (the same instructions in the same order: bit equality,
                # measured in all cases; the printed figures are 0)
                _err(vf, vp, tag + 'J fused vs pair')
                _err(bf, bp, tag + 'F fused vs pair')
                assert numpy.array_equal(vf, vp)
                assert numpy.array_equal(bf, bp)
                total += 1
                # the pair is what assemble() gives
                assert numpy.array_equal(vp, assemble(J).plane(0).cpu().numpy())
                assert numpy.array_equal(bp, assemble(F).get_local())
                # the same bits twice
                A2, b2 = asm.assemble()
                assert numpy.array_equal(vf, A2.plane(0).cpu().numpy())
                assert numpy.array_equal(bf, b2.cpu().numpy())
                # against the host evaluator
                Jh, Fh = bref.matrix(J), bref.vector(F)
                assert _err(Af.to_scipy(), Jh, tag + 'J fused vs host') < 1e-12
                assert _err(Ap.to_scipy(), Jh, tag + 'J pair vs host') < 1e-12
                assert _err(bf, Fh, tag + 'F fused vs host') < 1e-12
                assert _err(bp, Fh, tag + 'F pair vs host') < 1e-12
    assert total == 42


def _big_residual(V, u):
    '''J compiles to 57 instructions, F to 33, both together to 73 with the
    shared subtrees computed once: over the limit of 64.'''
    v = TestFunction(V)
    X = fem.SpatialCoordinate(V.mesh())
    return ((1 + u**2) * inner(grad(u), grad(v))
            + (sin(u) * X[0] + exp(u) * X[1]) * u.dx(0) * v
            + sqrt(1 + u * u) * v) * dx


def test_fallback_to_the_pair(hip):
    for degree in (1, 2):
        mesh = fem.UnitSquareMesh(8, 8)
        V = fem.FunctionSpace(mesh, 'CG', degree)
        u = nref.state(V)
        F = _big_residual(V, u)
        J = derivative(F, u)
        asm, vf, bf, A = _assembled(J, F, V, True)
        assert not asm.fused and [j[0] for j in asm.jobs] == ['matrix',
                                                              'vector']
        assert _err(A.to_scipy(), bref.matrix(J), 'fallback J vs host') < 1e-12
        assert _err(bf, bref.vector(F), 'fallback F vs host') < 1e-12
        # ... and a solve that takes that path
        f = fem.Constant(3.0)
        bcs = [fem.DirichletBC(V, fem.Expression('1.0 + x[0]*x[1]', degree=2),
                               'on_boundary')]
        v = TestFunction(V)
        uh = fem.interpolate(fem.Constant(1.0), V)
        info = fem.solve(_big_residual(V, uh) - f * v * dx == 0, uh, bcs)
        assert info.converged and info.fused is False
        ur = fem.interpolate(fem.Constant(1.0), V)
        res, its = nref.host_newton(_big_residual(V, ur) - f * v * dx, ur, bcs)
        assert info.iterations == its
        e = numpy.linalg.norm(uh.array() - ur.array()) \
            / numpy.linalg.norm(ur.array())
        print('fallback solve P%d: %r, rel l2 vs host Newton %.2e'
              % (degree, info, e))
        assert e < 1e-7


def test_solve_against_reference_newton(hip):
    '''-div((1 + u^2) grad u) = f with u_exact = sin(pi x) sin(pi y) and
    Dirichlet data, from u = 0: L2 orders within 0.1 of 2 (P1) and 3 (P2)
    over n = 8, 16, 32, asserted as the linear Poisson test asserts them; at
    n = 8 the iteration count of the host Newton (numpy evaluator, sparse LU)
    and its solution to 1e-7 relative l2, the bound of the linear solve
    against splu.'''
    for degree, order in ((1, 1.9), (2, 2.9)):
        errs = []
        for n in (8, 16, 32):
            V, u, F, bcs, exact = nref.quasilinear_problem(n, degree)
            info = fem.solve(F == 0, u, bcs)
            assert info.converged and info.fused
            assert info.method == 'gmres+ilu0'
            assert len(info.residuals) == info.iterations + 1
            assert len(info.linear_iterations) == info.iterations
            errs.append(fem.errornorm(exact, u))
            if n == 8:
                Vr, ur, Fr, bcr, _ = nref.quasilinear_problem(n, degree)
                res, its = nref.host_newton(Fr, ur, bcr)
                print('P%d residuals, device: %s' % (degree, info.residuals))
                print('P%d residuals, host:   %s' % (degree, res))
                assert info.iterations == its
                e = numpy.linalg.norm(u.array() - ur.array()) \
                    / numpy.linalg.norm(ur.array())
                print('P%d n = 8: %r; rel l2 vs host Newton %.2e'
                      % (degree, info, e))
                assert e < 1e-7
        rates = numpy.log2(numpy.array(errs[:-1]) / numpy.array(errs[1:]))
        print('P%d errors %s orders %s' % (degree, errs, rates))
        assert (rates > order).all()


def test_minimal_surface_solve(hip):
    '''-div(grad u / sqrt(1 + |grad u|^2)) = 1 with Dirichlet data: the
    Jacobian takes two programs (see above); iteration count and solution of
    the host Newton, 1e-7 relative l2 as for the other solves.'''
    for degree in (1, 2):
        pair = []
        for _ in range(2):
            V = fem.FunctionSpace(fem.UnitSquareMesh(8, 8), 'CG', degree)
            data = fem.Expression('0.1*x[0]*x[1]', degree=2)
            # (from the interpolated data: from u = 0 the jump at the
            # boundary makes the undamped iteration diverge, host and device)
            u, v = fem.interpolate(data, V), TestFunction(V)
            F = inner(grad(u), grad(v)) / sqrt(1 + dot(grad(u), grad(u))) * dx \
                - fem.Constant(1.0) * v * dx
            bcs = [fem.DirichletBC(V, data, 'on_boundary')]
            pair.append((u, F, bcs))
        (u, F, bcs), (ur, Fr, bcr) = pair
        info = fem.solve(F == 0, u, bcs)
        res, its = nref.host_newton(Fr, ur, bcr)
        e = numpy.linalg.norm(u.array() - ur.array()) \
            / numpy.linalg.norm(ur.array())
        print('minimal surface P%d: %r (host: %d iterations); rel l2 vs host '
              'Newton %.2e' % (degree, info, its, e))
        assert info.converged and not info.fused and info.iterations == its
        assert e < 1e-7


def _quasilinear(degree=2, n=8, extra=None, **kw):
    V, u, F, bcs, exact = nref.quasilinear_problem(n, degree)
    if extra is not None:
        F = F + extra(u, TestFunction(V))
    return fem.solve(F == 0, u, bcs, **kw), u, F, bcs


def test_newton_parameters_and_routes(hip, capsys):
    # non-symmetric with a convective term: GMRES + ILU(0), against the host
    def convection(u, v):
        return u * u.dx(0) * v * dx
    info, u, F, bcs = _quasilinear(extra=convection)
    assert info.converged and info.method == 'gmres+ilu0' and info.fused
    Vr, ur, Fr, bcr, _ = nref.quasilinear_problem(8, 2)
    Fr = Fr + convection(ur, TestFunction(Vr))
    res, its = nref.host_newton(Fr, ur, bcr)
    assert info.iterations == its
    e = numpy.linalg.norm(u.array() - ur.array()) / numpy.linalg.norm(ur.array())
    print('with convection: %r; rel l2 vs host Newton %.2e' % (info, e))
    assert e < 1e-7
    # chosen method: BiCGStab
    info_b, ub, _, _ = _quasilinear(solver_parameters={
        'newton_solver': {'linear_solver': 'bicgstab'}})
    assert info_b.converged and info_b.method.startswith('bicgstab')
    # a linear F: one iteration, the solution of solve(a == L)
    mesh = fem.UnitSquareMesh(8, 8)
    V = fem.FunctionSpace(mesh, 'CG', 2)
    f = fem.Expression('2.0*pi*pi*sin(pi*x[0])*sin(pi*x[1])', degree=4)
    bcs = [fem.DirichletBC(V, fem.Expression('x[0]*x[1]', degree=2),
                           'on_boundary')]
    v, du = TestFunction(V), TrialFunction(V)
    ul, un = fem.Function(V), fem.Function(V)
    fem.solve(inner(grad(du), grad(v)) * dx == f * v * dx, ul, bcs)
    info = fem.solve(inner(grad(un), grad(v)) * dx - f * v * dx == 0, un, bcs)
    assert info.converged and info.iterations == 1 and info.method == 'cg'
    e = numpy.linalg.norm(un.array() - ul.array()) / numpy.linalg.norm(ul.array())
    print('linear F: %r; rel l2 vs solve(a == L) %.2e' % (info, e))
    assert e < 1e-10
    # damping: slower, the same solution
    full, u1, _, _ = _quasilinear()
    half, u2, _, _ = _quasilinear(solver_parameters={
        'newton_solver': {'relaxation_parameter': 0.5}})
    print('relaxation 1.0: %d iterations, 0.5: %d' % (full.iterations,
                                                     half.iterations))
    assert half.converged and half.iterations > full.iterations
    assert numpy.linalg.norm(u2.array() - u1.array()) \
        < 1e-7 * numpy.linalg.norm(u1.array())
    # one iteration is not enough
    with pytest.raises(_hip.NotConverged):
        _quasilinear(solver_parameters={
            'newton_solver': {'maximum_iterations': 1}})
    info, _, _, _ = _quasilinear(solver_parameters={'newton_solver': {
        'maximum_iterations': 1, 'error_on_nonconvergence': False}})
    assert info.converged is False and info.iterations == 1
    assert len(info.residuals) == 2
    # J= the default, given: the same bits
    V, u3, F3, bcs3, _ = nref.quasilinear_problem(8, 2)
    info3 = fem.solve(F3 == 0, u3, bcs3, J=derivative(F3, u3))
    assert info3.fused and info3.residuals == full.residuals
    assert numpy.array_equal(u3.array(), u1.array())
    # report: one line per iteration (residual evaluation)
    capsys.readouterr()
    message.set_log_active(True)
    try:
        info, _, _, _ = _quasilinear(solver_parameters={
            'newton_solver': {'report': True}})
    finally:
        message.set_log_active(False)
    lines = [ln for ln in capsys.readouterr().out.splitlines()
             if ln.strip().startswith('Newton iteration')]
    assert len(lines) == info.iterations + 1
    # assemble_system takes a derived J as it is
    A, b = fem.assemble_system(derivative(F3, u3), F3, bcs3)
    assert A.kind == 0 and b.get_local().shape == (V.N,)


def test_heat_conduction_with_water_conductivity(hip):
    '''Steady conduction -div(kappa(theta) grad theta) = f in water, kappa
    from flow_amd.materials, theta between 280 K and 340 K on the boundary.
    Energy balance: int f dx = -int kappa dtheta/dn ds up to the
    discretisation error of the boundary flux of a P2 solution, O(h^2): the
    imbalance must fall by more than 2 from n = 8 to n = 16 (4 expected) and
    stay under 5 % of the source at n = 16.'''
    imbalance = []
    for n in (8, 16):
        mesh = fem.UnitSquareMesh(n, n)
        V = fem.FunctionSpace(mesh, 'CG', 2)
        theta = fem.interpolate(fem.Constant(310.0), V)
        v = TestFunction(V)
        kappa = materials.thermal_conductivity(theta)
        f = fem.Expression('100.0*(1.0 + x[0])', degree=1)
        bcs = [fem.DirichletBC(
            V, fem.Expression('310.0 + 30.0*cos(pi*x[0])*cos(pi*x[1])',
                              degree=4), 'on_boundary')]
        F = kappa * inner(grad(theta), grad(v)) * dx - f * v * dx
        info = fem.solve(F == 0, theta, bcs)
        assert info.converged and info.fused and info.iterations >= 2
        t = theta.array()
        assert t.min() > 279.0
        nrm = fem.FacetNormal(mesh)
        source = assemble(f * dx(mesh))
        flux = assemble(-kappa * dot(grad(theta), nrm) * ds(mesh))
        print('n = %d: %r; theta in [%.1f, %.1f]; source %.6e, boundary flux '
              '%.6e, imbalance %.3e' % (n, info, t.min(), t.max(), source,
                                        flux, abs(source - flux) / source))
        imbalance.append(abs(source - flux) / source)
    assert imbalance[1] < 0.5 * imbalance[0]
    assert imbalance[1] < 0.05
