# -*- coding: utf-8 -*-
'''
Newton's method on a Taylor-Hood space on the GPU (fem.mixed_derivatives;
flow_amd/fem/mixed.py, csrc/mixed_kernels.hip): flow_mixed_upper_rhs and
BlockTriangularPreconditioner.apply_fused bit for bit against the composed
sequence, MixedNewtonAssembler bit for bit against assemble(), derivative()
against a hand-written Jacobian, and solve(F == 0, w, bcs) step by step against
the host loop of tests/mixed_newton_reference.py (sparse LU) on Kovasznay's
flow and on a Forchheimer-Brinkman insert; determinism.

Measured on an MI355X on the first run of these tests (relative max-norm):
  derivative(F, w) against the hand-written J written part by part as
  derivative() leaves its parts: the part tables are identical
  (tests/test_mixed_newton_host.py), so equal bits are required.  Against the
  same J written as five separate integrals (the two convective terms added
    by an axpby, not inside one element kernel): uu 1.99e-16 (216 cells),
  1.69e-16 (1648 cells); the coupling blocks 0.
  Kovasznay, Re = 40, RectangleMesh 16 x 16, 5 Newton steps (139 .. 151 FGMRES
  iterations each), each step against the host loop's step: u <= 2.17e-12,
  p <= 6.62e-12 (both at the first steps; 3.4e-15 / 5.1e-14 at the last).
  |F| 1.038, 4.796e-1, 7.031e-2, 1.320e-3, 4.329e-7, 1.355e-13 on both sides.
  Against the exact fields Newton and 26 Picard steps both give u 7.3796e-4,
  p 1.7235e-2: the discretisation error.
  Forchheimer-Brinkman insert, relaxation 0.8, 14 steps (81 .. 88
  iterations): u <= 1.14e-12, p <= 1.62e-12 (step 1; 2e-16 at the end).
The bounds are 10x the largest measured figure of their kind, capped by 1e-12
(matrices) and by the field-parity bound PARITY (solves).
'''
import numpy
import pytest
import torch

from flow_amd import fem, _hip, device
from flow_amd.fem import (
    TestFunctions, TrialFunctions, assemble, solve, derivative, dx, dot, inner,
    grad, div, sqrt,
    )
from flow_amd.fem import ops, mixed
from flow_amd.fem.bcs import FixedDofsBC

import mixed_newton_reference as ref
from test_mixed_gmres_gpu import (
    _meshes, _space, PAIRS, _profile, _problem, _oseen, _rel, _dev,
    _vectors, _Side, LONG, PARITY, PICARD_STEPS,
    )

pytestmark = pytest.mark.gpu

MATRIX_CAP = 1e-12
# 10x the measured figures of the header, capped
SPLIT_J_BOUND = min(MATRIX_CAP, 10 * 1.99e-16)
KOVASZNAY_U = min(PARITY, 10 * 2.17e-12)
KOVASZNAY_P = min(PARITY, 10 * 6.62e-12)
INSERT_U = min(PARITY, 10 * 1.14e-12)
INSERT_P = min(PARITY, 10 * 1.62e-12)


@pytest.fixture(autouse=True)
def _switches_on():
    with fem.mixed_arguments(True), fem.vector_arguments(True), \
            fem.facet_arguments(True), fem.cell_subdomains(True), \
            fem.mixed_gmres(True), fem.mixed_derivatives(True):
        yield


def _composed(A, sinv, r):
    '''The first half of BlockTriangularPreconditioner.apply, launch by
    launch: (z_p, ru).'''
    n2, nv = A.W.size(), A.W.N
    zp = torch.full((A.P.N,), float('nan'), dtype=torch.float64,
                    device=r.device)
    ops.vmul(r[n2:], sinv, zp)
    ru = ops.copy(torch.full((n2,), float('nan'), dtype=torch.float64,
                             device=r.device), r[:n2])
    tmp = device.empty(nv)
    for c in range(2):
        if A.up[c] is not None:
            A.up[c].apply(zp, tmp)
            ops.axpby(-1.0, tmp, 1.0, ru[c * nv:(c + 1) * nv])
    return zp, ru


def _fused(A, sinv, r):
    zp = torch.full((A.P.N,), float('nan'), dtype=torch.float64,
                    device=r.device)
    ru = torch.full((A.W.size(),), float('nan'), dtype=torch.float64,
                    device=r.device)
    return mixed.upper_rhs(A, sinv, r, zp, ru)


# -- 1. the kernel ------------------------------------------------------------------
def test_upper_rhs_bits(hip):
    for mesh in _meshes():
        for kv, kp in PAIRS:
            WP = _space(mesh, kv, kp)
            W = WP.sub(0)
            wu = fem.split(_profile(WP, mesh, 1.5))[0]
            (x0, y0), (x1, y1) = mesh.points.min(axis=0), \
                mesh.points.max(axis=0)
            tol = 1e-10 * (x1 - x0)
            walls = _Side(lambda x: (x[0] > x0 + tol) & (x[0] < x1 - tol))
            (v, q) = TestFunctions(WP)
            A, _ = mixed.assemble_system(
                _oseen(WP, fem.Constant(0.05), wu),
                inner(fem.Constant((0.0, 0.0)), v) * dx,
                [fem.DirichletBC(WP.sub(0), fem.Constant((0.0, 0.0)), walls)])
            tag = '%d cells P%d/P%d' % (mesh.num_cells(), kv, kp)
            print('%s: %d velocity dofs, %d velocity tiles'
                  % (tag, W.N, A.fused().nvtiles))
            variants = {
                'both planes': A,
                'up0 only': mixed.MixedMatrix(WP, A.uu, A.pp, [A.up[0], None],
                                              A.pu),
                'up1 only': mixed.MixedMatrix(WP, A.uu, A.pp, [None, A.up[1]],
                                              A.pu),
                'no plane': mixed.MixedMatrix(WP, A.uu, A.pp, None, A.pu),
                }
            rng = numpy.random.RandomState(3)
            sinv = _dev(rng.uniform(0.1, 10.0, A.P.N)
                        * rng.choice([-1.0, 1.0], A.P.N))
            for name, B in variants.items():
                for rs in _vectors(A.size, 13):
                    r = _dev(rs)
                    zp0, ru0 = _composed(B, sinv, r)
                    zp1, ru1 = _fused(B, sinv, r)
                    assert not torch.isnan(zp0).any()
                    assert not torch.isnan(ru0).any()
                    assert torch.equal(zp1, zp0), (tag, name)
                    assert torch.equal(ru1, ru0), (tag, name)
                    # (the coupling changes the velocity rows)
                    if name != 'no plane':
                        assert not torch.equal(ru0, r[:A.W.size()])
                    # a second call gives the same bits
                    zp2, ru2 = _fused(B, sinv, r)
                    assert torch.equal(zp2, zp1) and torch.equal(ru2, ru1)
            # ru aliasing r: refused, nothing launched
            r = _dev(_vectors(A.size, 14)[0])
            zp = device.empty(A.P.N)
            before = _hip.launch_count()
            with pytest.raises(ValueError, match='overlaps'):
                mixed.upper_rhs(A, sinv, r, zp, r[:A.W.size()])
            with pytest.raises(ValueError, match='overlaps'):
                mixed.upper_rhs(A, sinv, r, r[A.W.size():],
                                device.empty(A.W.size()))
            assert _hip.launch_count() == before


# -- 2. the preconditioner ------------------------------------------------------------
def test_preconditioner_apply_fused_bits(hip):
    for which in ('square', 'channel'):
        mesh, WP, bcs, pin, dsm, dxm, w0 = _problem(which)
        (v, q) = TestFunctions(WP)
        A, _ = mixed.assemble_system(
            _oseen(WP, fem.Constant(0.05), fem.split(w0)[0]),
            inner(fem.Constant((0.0, 0.0)), v) * dx, bcs)
        for velocity in ('ilu0', 'jacobi'):
            M = mixed.BlockTriangularPreconditioner(A, velocity)
            for rs in _vectors(A.size, 17):
                r = _dev(rs)
                z0 = M.apply(r, torch.full_like(r, float('nan')))
                z1 = M.apply_fused(r, torch.full_like(r, float('nan')))
                assert not torch.isnan(z0).any()
                assert torch.equal(z1, z0), (which, velocity)


# -- 3. the assembler -----------------------------------------------------------------
def _residual(WP, w, nu=0.05):
    (u, p) = fem.split(w)
    (v, q) = TestFunctions(WP)
    f = fem.Expression(('sin(3.0*x[1])', 'x[0]*x[1]'), degree=2)
    F = fem.Constant(nu) * inner(grad(u), grad(v)) * dx \
        + dot(dot(grad(u), u), v) * dx - p * div(v) * dx - q * div(u) * dx \
        - inner(f, v) * dx
    return F, u, p, v, q


def _perturbed(WP, mesh, seed):
    '''The Poiseuille profile plus a smooth perturbation of u and p.'''
    w = _profile(WP, mesh)
    W, P = WP.sub(0), WP.sub(1)
    xu, xp = W.layout.dof_coords, P.layout.dof_coords
    vals = w.array()
    a = 0.1 * (seed + 1)
    vals[:W.N] += a * numpy.sin(3.0 * xu[:, 0]) * numpy.cos(2.0 * xu[:, 1])
    vals[W.N:2 * W.N] += a * numpy.cos(xu[:, 0] + 2.0 * xu[:, 1])
    vals[2 * W.N:] += a * numpy.sin(2.0 * xp[:, 0] - xp[:, 1])
    return vals


def _same_blocks(A, B, tag):
    names = [k for k, _ in B.blocks()]
    assert [k for k, _ in A.blocks()] == names
    for (k, X), (_, Y) in zip(A.blocks(), B.blocks()):
        n = X.layout.nnz
        if k == 'uu':
            for pl in range(4):
                assert torch.equal(X.plane(pl)[:n], Y.plane(pl)[:n]), (tag, k)
        elif k == 'pp':
            assert torch.equal(X.vals[:n], Y.vals[:n]), (tag, k)
        else:
            assert torch.equal(X.plane(), Y.plane()), (tag, k)


def test_assembler_bits_and_frozen_blocks(hip):
    mesh = fem.UnitSquareMesh(12, 9)
    WP = _space(mesh, 2, 1)
    n2 = WP.sub(0).size()
    w = fem.Function(WP)
    F, u, p, v, q = _residual(WP, w)
    for name, form in (('Navier-Stokes', F),
                       ('with -p*p*div(v)', F - p * p * div(v) * dx)):
        J = derivative(form, w)
        asm = mixed.MixedNewtonAssembler(J, form, WP, w=w)
        if name == 'Navier-Stokes':
            assert asm.frozen == ('up0', 'up1', 'pu0', 'pu1')
        else:
            assert asm.frozen == ('pu0', 'pu1')
        held = None
        for seed in range(3):
            w.set_array(_perturbed(WP, mesh, seed))
            A, b = asm.assemble()
            _same_blocks(A, assemble(J), (name, seed))
            want = assemble(form).data
            assert torch.equal(b[:n2], want[:n2]), (name, seed)
            assert torch.equal(b[n2:], want[n2:]), (name, seed)
            # the buffers live as long as the object
            ptrs = [X.vals.data_ptr() for _, X in A.blocks()] + [b.data_ptr()]
            assert held is None or held == ptrs
            held = ptrs


# -- 4. derivative() against a hand-written Jacobian ------------------------------------
def test_derivative_against_hand_written_jacobian(hip):
    worst = {}
    for mesh in _meshes():
        WP = _space(mesh, 2, 1)
        w = fem.Function(WP)
        w.set_array(_perturbed(WP, mesh, 1))
        F, u, p, v, q = _residual(WP, w)
        (du, dp) = TrialFunctions(WP)
        nu = fem.Constant(0.05)
        J = assemble(derivative(F, w))
        by_parts = assemble(
            nu * inner(grad(du), grad(v)) * dx
            + (dot(dot(grad(du), u), v) + dot(dot(grad(u), du), v)) * dx
            - dp * div(v) * dx - q * div(du) * dx)
        # identical part tables (the host test): equal bits
        _same_blocks(J, by_parts, mesh.num_cells())
        split = assemble(
            nu * inner(grad(du), grad(v)) * dx
            + dot(dot(grad(du), u), v) * dx + dot(dot(grad(u), du), v) * dx
            - dp * div(v) * dx - q * div(du) * dx)
        for (k, X), (_, Y) in zip(J.blocks(), split.blocks()):
            e = abs(X.to_scipy() - Y.to_scipy()).max() \
                / abs(Y.to_scipy()).max()
            print('derivative against five integrals, %d cells, %s: %.2e'
                  % (mesh.num_cells(), k, e))
            worst[k] = max(worst.get(k, 0.0), e)
    print('worst per block: %s' % worst)
    assert max(worst.values()) < SPLIT_J_BOUND


# -- 5. / 6. solves ---------------------------------------------------------------------
def _kovasznay():
    re = 40.0
    lam = re / 2.0 - numpy.sqrt(re * re / 4.0 + 4.0 * numpy.pi ** 2)
    mesh = fem.RectangleMesh(fem.Point(-0.5, -0.5), fem.Point(1.0, 1.5), 16, 16)
    WP = _space(mesh, 2, 1)
    W, P = WP.sub(0), WP.sub(1)
    two_pi = 2.0 * numpy.pi
    ue = fem.Expression(
        ('1.0 - exp(%.17g*x[0])*cos(%.17g*x[1])' % (lam, two_pi),
         '%.17g*exp(%.17g*x[0])*sin(%.17g*x[1])' % (lam / two_pi, lam,
                                                     two_pi)), degree=4)
    pe = lambda x: 0.5 * (1.0 - numpy.exp(2.0 * lam * x[:, 0]))   # noqa: E731
    # one pinned pressure dof: the vertex at the lower left corner
    pin = int(numpy.abs(P.layout.dof_coords - [-0.5, -0.5]).sum(axis=1).argmin())
    bcs = [fem.DirichletBC(WP.sub(0), ue, 'on_boundary'),
           FixedDofsBC(WP.sub(1), [pin], pe(P.layout.dof_coords[[pin]]))]
    xu, xp = W.layout.dof_coords, P.layout.dof_coords
    exact_u = numpy.concatenate([
        1.0 - numpy.exp(lam * xu[:, 0]) * numpy.cos(two_pi * xu[:, 1]),
        lam / two_pi * numpy.exp(lam * xu[:, 0]) * numpy.sin(two_pi * xu[:, 1])])
    return re, WP, bcs, exact_u, pe(xp)


def _navier_stokes(WP, w, nu):
    '''(F, hand-written J) over the views of w.'''
    (u, p) = fem.split(w)
    (v, q) = TestFunctions(WP)
    (du, dp) = TrialFunctions(WP)
    nu = fem.Constant(nu)
    F = nu * inner(grad(u), grad(v)) * dx + dot(dot(grad(u), u), v) * dx \
        - p * div(v) * dx - q * div(u) * dx \
        - inner(fem.Constant((0.0, 0.0)), v) * dx
    J = nu * inner(grad(du), grad(v)) * dx + dot(dot(grad(du), u), v) * dx \
        + dot(dot(grad(u), du), v) * dx - dp * div(v) * dx \
        - q * div(du) * dx
    return F, J


def _steps_against_host(build, WP, bcs, ns, tag):
    '''The solve from a zero start against the host loop.  build(w): (F,
    hand-written J) over w.  The device solve runs once in one call (its
    NewtonInfo is returned) and once step by step -- 'maximum_iterations': 1
    per call, every call starting from the iterate the one before left -- so
    that every iterate is compared with the host's.  Returns (worst u, worst
    p, info, device field, host residuals).'''
    n2 = WP.sub(0).size()
    wh = fem.Function(WP)
    Fh, Jh = build(wh)
    iterates, hres = ref.newton(Fh, Jh, wh, bcs,
                                ns.get('relaxation_parameter', 1.0))
    w = fem.Function(WP)
    F, _ = build(w)
    info = solve(F == 0, w, bcs, solver_parameters={'newton_solver': ns})
    final = w.array()
    ws = fem.Function(WP)
    Fs, _ = build(ws)
    one = dict(ns)
    one.update({'maximum_iterations': 1, 'error_on_nonconvergence': False})
    worst_u = worst_p = 0.0
    for k in range(1, len(iterates)):
        step = solve(Fs == 0, ws, bcs, solver_parameters={'newton_solver': one})
        assert step.iterations == 1
        xg = ws.array()
        eu = _rel(xg[:n2], iterates[k][:n2])
        ep = _rel(xg[n2:], iterates[k][n2:])
        print('%s step %d: %3d its, |F| device %.3e host %.3e; against the '
              'host loop u %.2e p %.2e'
              % (tag, k, step.linear_iterations[0], step.residuals[0],
                 hres[k - 1], eu, ep))
        worst_u, worst_p = max(worst_u, eu), max(worst_p, ep)
    print('%s: worst u %.2e p %.2e; residuals device %s host %s'
          % (tag, worst_u, worst_p, ['%.3e' % r for r in info.residuals],
             ['%.3e' % r for r in hres]))
    # the one-call solve against the host's last iterate
    eu, ep = _rel(final[:n2], iterates[-1][:n2]), \
        _rel(final[n2:], iterates[-1][n2:])
    print('%s: one call against the host loop u %.2e p %.2e; same bits as '
          'step by step: %s' % (tag, eu, ep,
                                numpy.array_equal(final, ws.array())))
    worst_u, worst_p = max(worst_u, eu), max(worst_p, ep)
    return worst_u, worst_p, info, final, hres


def _newton_checks(info, hres, quadratic):
    '''Newton's own iterations against the host loop's sequence.'''
    res = info.residuals
    assert info.converged
    assert res[-1] < 1e-10 or res[-1] / res[0] < 1e-9
    assert info.iterations == len(hres) - 1 == len(res) - 1
    assert info.method == 'fgmres+ilu0' and info.route == 'by_parts'
    assert len(info.linear_iterations) == info.iterations
    if not quadratic:
        return
    # once below 1e-2 |F0|: r_next <= C r^2, C from the host's own sequence
    # (the largest ratio it shows in that regime, doubled: the last residual
    # of either loop sits on the rounding floor of the assembly)
    ratios = [hres[k + 1] / hres[k] ** 2 for k in range(len(hres) - 1)
              if hres[k] < 1e-2 * hres[0]]
    assert ratios
    C = 2.0 * max(ratios)
    for k in range(len(res) - 1):
        if res[k] < 1e-2 * res[0]:
            print('r[%d] = %.3e <= C r[%d]^2 = %.3e' % (k + 1, res[k + 1], k,
                                                       C * res[k] ** 2))
            assert res[k + 1] <= C * res[k] ** 2


def test_newton_kovasznay(hip):
    re, WP, bcs, exact_u, exact_p = _kovasznay()
    n2 = WP.sub(0).size()
    ns = {'krylov_solver': dict(LONG)}
    worst_u, worst_p, info, xg, hres = _steps_against_host(
        lambda w: _navier_stokes(WP, w, 1.0 / re), WP, bcs, ns, 'Kovasznay')
    assert info.frozen == ('up0', 'up1', 'pu0', 'pu1')
    _newton_checks(info, hres, True)
    # the Picard loop of tests/test_mixed_gmres_gpu.py::test_picard_kovasznay
    (v, q) = TestFunctions(WP)
    L = inner(fem.Constant((0.0, 0.0)), v) * dx
    old, wp = fem.Function(WP), fem.Function(WP)
    a = _oseen(WP, fem.Constant(1.0 / re), fem.split(old)[0])
    for _ in range(PICARD_STEPS):
        solve(a == L, wp, bcs, solver_parameters={'krylov_solver': dict(LONG)})
        old.set_array(wp.array())
    xp = wp.array()
    figures = [(_rel(x[:n2], exact_u), _rel(x[n2:], exact_p))
               for x in (xg, xp)]
    print('Kovasznay: Newton %d iterations (%s linear); against the exact '
          'fields: Newton u %.4e p %.4e, Picard (%d steps) u %.4e p %.4e'
          % ((info.iterations, info.linear_iterations) + figures[0]
             + (PICARD_STEPS,) + figures[1]))
    assert figures[0][0] <= 1.01 * figures[1][0]
    assert figures[0][1] <= 1.01 * figures[1][1]
    assert worst_u < KOVASZNAY_U and worst_p < KOVASZNAY_P


def _insert(which='square'):
    mesh, WP, bcs, pin, dsm, dxm, w0 = _problem(which)

    def build(w):
        F, J = _navier_stokes(WP, w, 0.05)
        (u, p) = fem.split(w)
        (v, q) = TestFunctions(WP)
        (du, dp) = TrialFunctions(WP)
        beta = fem.Constant(3.0)
        speed = sqrt(dot(u, u) + 1e-12)
        # (one quadrature degree for the term and its hand-written
        # derivative: derivative() keeps the degree of the part it came from,
        # the estimate for the hand-written integrand is another, and the
        # integrand is no polynomial -- the two Jacobians then differ by
        # 1e-5 and every Newton step with them)
        dxi = dxm(1, degree=6)
        F = F + beta * speed * dot(u, v) * dxi \
            - dot(fem.Constant((-0.5, 0.25)), v) * dsm(2)
        J = J + beta * (speed * dot(du, v)
                        + dot(u, du) / speed * dot(u, v)) * dxi
        return F, J
    return WP, bcs, build


def test_newton_forchheimer_brinkman_insert(hip):
    WP, bcs, build = _insert()
    ns = {'relaxation_parameter': 0.8}
    worst_u, worst_p, info, xg, hres = _steps_against_host(
        build, WP, bcs, ns, 'insert')
    assert info.frozen == ('up0', 'up1', 'pu0', 'pu1')
    _newton_checks(info, hres, False)
    assert worst_u < INSERT_U and worst_p < INSERT_P


# -- 7. determinism ---------------------------------------------------------------------
def test_the_same_solve_gives_the_same_bits(hip):
    WP, bcs, build = _insert()
    runs = []
    for _ in range(2):
        w = fem.Function(WP)
        F, _ = build(w)
        info = solve(F == 0, w, bcs, solver_parameters={
            'newton_solver': {'relaxation_parameter': 0.8}})
        runs.append((w.array(), list(info.residuals),
                     list(info.linear_iterations)))
    assert numpy.array_equal(runs[0][0], runs[1][0])
    assert runs[0][1] == runs[1][1] and runs[0][2] == runs[1][2]


def test_refusals_on_the_device(hip):
    WP, bcs, build = _insert()
    w = fem.Function(WP)
    F, J = build(w)
    with pytest.raises(ValueError, match="'ilu0' or 'jacobi'"):
        solve(F == 0, w, bcs, solver_parameters={
            'newton_solver': {'preconditioner': 'two_level'}})
    with fem.mixed_gmres(False):
        with pytest.raises(NotImplementedError, match='mixed_gmres'):
            solve(F == 0, w, bcs)
    with fem.mixed_derivatives(False):
        with pytest.raises(NotImplementedError, match='scalar and vector'):
            solve(F == 0, w, bcs)
    # 'jacobi' and a hand-written J are taken
    info = solve(F == 0, w, bcs, J=J, solver_parameters={'newton_solver': {
        'relaxation_parameter': 0.8, 'preconditioner': 'jacobi',
        'krylov_solver': dict(LONG)}})
    assert info.converged and info.method == 'fgmres+jacobi'
