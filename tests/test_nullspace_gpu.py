# -*- coding: utf-8 -*-
'''
Nullspaces on the GPU (flow_amd/fem/nullspace.py, csrc/nullspace_kernels.hip):
flow_deflate bit for bit against flow_multi_dot and the composed sequence and
within the rounding bound of the extended-precision model; solve(...,
nullspace=ns) against the bordered sparse LU of tests/nullspace_reference.py
for pure Neumann Poisson, a free elastic body, enclosed Stokes (MINRES and
FGMRES), enclosed Oseen and enclosed Navier-Stokes by Newton's method; the
refusals; and nullspace=None against the call without the keyword.
'''
import numpy
import pytest
import torch

from flow_amd import fem, _hip, device
from flow_amd.fem import (
    TestFunction, TrialFunction, TestFunctions, TrialFunctions,
    assemble_system, solve, dx, Measure, MeshFunction, dot, inner, grad, div,
    sym,
    )
from flow_amd.fem import ops
from flow_amd.fem.bcs import FixedDofsBC

import nullspace_reference as ref
from test_mixed_gmres_gpu import (
    _space, _oseen, _stokes, _rel, _Side, _profile, _cases, LONG, PARITY,
    )

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
# the bordered LU's own relative residual (checked for every reference)
LU_RESIDUAL = 1e-13

# Against the bordered LU, relative max-norm, solver tolerance relative 1e-12:
# the convention of tests/test_mixed_gmres_gpu.py -- 10x the figure measured on
# the first MI355X run, capped by the field-parity bound.  The margin covers
# iteration-count jitter from rounding.  Measured on the first MI355X run
# (iterations):
#   Neumann Poisson 8 x 6    P1 2.01e-14 (43), shifted source 5.13e-14
#                            P2 4.54e-14 (95), shifted source 6.52e-14
#   free elastic body P2     1.73e-13 (155)
#   enclosed Stokes            u         p
#     minres jacobi          9.01e-13  1.59e-12 (158)
#     minres two_level       1.25e-12  1.35e-12 (156)
#     fgmres ilu0            1.76e-12  1.85e-12 (47)
#     fgmres jacobi          2.41e-12  1.90e-12 (125)
#   enclosed Oseen
#     fgmres ilu0            1.55e-11  1.94e-11 (50)
#     fgmres jacobi          4.59e-12  1.53e-12 (108)
#   enclosed Newton, 3 steps (52, 52, 53), each against the host loop's step:
#                            7.68e-12  1.20e-10 (both at step 1; 1.7e-16 /
#                            3.1e-14 at step 3); |F| 11.31, 2.324e-1,
#                            1.211e-5, 2.15e-13 on both sides
# Stokes and Oseen share one pair of bounds: the largest figure of the kind.
POISSON_BOUND = min(PARITY, 10 * 6.52e-14)
ELASTIC_BOUND = min(PARITY, 10 * 1.73e-13)
STOKES_U = min(PARITY, 10 * 1.55e-11)
STOKES_P = min(PARITY, 10 * 1.94e-11)
NEWTON_U = min(PARITY, 10 * 7.68e-12)
NEWTON_P = min(PARITY, 10 * 1.20e-10)

MANY = {'relative_tolerance': 1e-12, 'maximum_iterations': 4000}


@pytest.fixture(autouse=True)
def _switches_on():
    with fem.mixed_arguments(True), fem.vector_arguments(True), \
            fem.facet_arguments(True), fem.cell_subdomains(True), \
            fem.mixed_gmres(True), fem.mixed_derivatives(True), \
            fem.vector_derivatives(True):
        yield


def _dev(a):
    return device.to_device(numpy.ascontiguousarray(a, dtype=numpy.float64))


def _host(t):
    return device.to_host(t).numpy().copy()


# -- 1. the kernel ------------------------------------------------------------------
# launch 1 gives a workgroup 256 entry pairs: 512 rows
ROWS = 512
SIZES = [
    1, 2, ROWS - 1, ROWS, ROWS + 1,
    2 * ROWS + 37,               # three blocks, the last one ragged
    256 * ROWS + 515,            # more than one LDS tile of block partials
    1024 * ROWS + 3,             # the grid stride of launch 1 runs twice
    2048 * ROWS + 5,             # the grid stride of launch 2 runs twice
    ]


def _operands(n, seed):
    rng = numpy.random.RandomState(seed)
    Z = rng.standard_normal((8, n)) * 10.0 ** rng.uniform(-2, 2, (8, 1))
    x = rng.standard_normal(n) * 10.0 ** rng.uniform(-2, 2, n)
    ld = n + (n & 1) + 2
    store = numpy.full(8 * ld, numpy.nan)
    for j in range(8):
        store[j * ld:j * ld + n] = Z[j]
    return Z, x, ld, _dev(store)


def _deflate(hip, n, k, Zd, ld, xd, work, coef):
    _hip.check(hip.flow_deflate(
        n, k, _hip.f64(Zd), ld, _hip.f64(xd, n), _hip.f64(work),
        None if coef is None else _hip.f64(coef, k), _hip.stream()))


def _composed(hip, n, k, Zd, ld, xd, work):
    '''flow_multi_dot, a negation, flow_combine(base = x) into a second
    buffer: (coefficients, result).'''
    c = device.empty(k)
    _hip.check(hip.flow_multi_dot(n, k, _hip.f64(Zd), ld, _hip.f64(xd, n),
                                  _hip.f64(work), _hip.f64(c, k),
                                  _hip.stream()))
    minus = torch.neg(c)
    out = device.empty(n)
    _hip.check(hip.flow_combine(n, k, _hip.f64(Zd), ld, 1, _hip.f64(minus, k),
                                _hip.f64(xd, n), _hip.f64(out, n), ld,
                                _hip.stream()))
    return _host(c), _host(out)


@pytest.mark.parametrize('n', SIZES)
def test_deflate_bits_and_bound(hip, n):
    Z, x, ld, Zd = _operands(n, n % 1000)
    work = device.empty(8 * _hip.MULTI_DOT_BLOCKS)
    coefs = {}
    for k in (1, 3, 8):
        want_c, want_x = _composed(hip, n, k, Zd, ld, _dev(x), work)
        xd, coef = _dev(x), device.zeros(k)
        before = _hip.launch_count()
        _deflate(hip, n, k, Zd, ld, xd, work, coef)
        assert _hip.launch_count() == before + 2
        got_c, got_x = _host(coef), _host(xd)
        assert numpy.array_equal(got_c, want_c), (n, k, got_c, want_c)
        bad = numpy.nonzero(got_x != want_x)[0]
        assert len(bad) == 0, (n, k, len(bad), bad[:8])
        # two calls, and a call without coef: the same bits
        x2 = _dev(x)
        _deflate(hip, n, k, Zd, ld, x2, work, None)
        assert numpy.array_equal(_host(x2), got_x)
        # against the extended-precision model
        xl, cl = ref.deflate(Z[:k], x)
        xb, cb = ref.deflate_bound(Z[:k], x)
        ec = numpy.abs(got_c - cl.astype(float)) / cb
        ex = numpy.abs(got_x - xl.astype(float)) / xb
        print('n %8d k %d: coef error / bound %.3f, x error / bound %.3f'
              % (n, k, ec.max(), ex.max()))
        assert ec.max() <= 1.0 and ex.max() <= 1.0
        coefs[k] = got_c
    # a column's coefficient depends on n, the column and x alone
    assert coefs[3][0] == coefs[1][0] == coefs[8][0]
    assert numpy.array_equal(coefs[8][:3], coefs[3])
    coef = device.zeros(1)
    _deflate(hip, n, 1, Zd[5 * ld:], ld, _dev(x), work, coef)
    assert _host(coef)[0] == coefs[8][5]
    # the padding of the store (NaN) was never read, and Z is untouched
    store = _host(Zd)
    for j in range(8):
        assert numpy.array_equal(store[j * ld:j * ld + n], Z[j])


def test_deflate_refusals(hip):
    n = 1061
    Z, x, ld, Zd = _operands(n, 5)
    work = device.empty(8 * _hip.MULTI_DOT_BLOCKS)
    coef = device.zeros(9)
    buf = device.zeros(n + 8)
    before = _hip.launch_count()
    with pytest.raises(ValueError, match='aligned'):
        _deflate(hip, n, 3, Zd, ld, buf[1:], work, coef)
    with pytest.raises(ValueError, match='aligned'):
        _deflate(hip, n, 3, Zd[1:], ld, buf, work, coef)
    with pytest.raises(ValueError, match='ldz'):
        _deflate(hip, n, 3, Zd, n - 1, buf, work, coef)
    with pytest.raises(ValueError, match='x overlaps Z'):
        _deflate(hip, n, 3, Zd, ld, Zd[2 * ld:], work, coef)
    with pytest.raises(ValueError, match='work overlaps x'):
        _deflate(hip, n, 1, Zd, ld, work, work, coef)
    with pytest.raises(ValueError, match='work overlaps Z'):
        _deflate(hip, n, 3, Zd, ld, buf, Zd, coef)
    with pytest.raises(ValueError, match='coef overlaps x'):
        _deflate(hip, n, 3, Zd, ld, buf, work, buf[4:])
    with pytest.raises(ValueError, match='coef overlaps work'):
        _deflate(hip, n, 3, Zd, ld, buf, work, work[8:])
    with pytest.raises(ValueError, match='k <= 8'):
        _deflate(hip, n, 9, Zd, ld, buf, work, coef)
    assert hip.flow_deflate(0, 3, None, 0, None, None, None, None) == 0
    assert hip.flow_deflate(n, 0, None, ld, None, None, None, None) == 0
    assert _hip.launch_count() == before


def test_basis_on_the_device(hip):
    '''VectorSpaceBasis.orthogonalize / coefficients on a Vector, a Function
    and a device array, with and without a support.'''
    mesh = fem.UnitSquareMesh(8, 6)
    WP = _space(mesh, 2, 1)
    W, P = WP.taylor_hood()
    ns = fem.constant_nullspace(WP)
    rng = numpy.random.RandomState(3)
    vals = rng.standard_normal(WP.size())
    w = fem.Function(WP)
    w.set_array(vals)
    c = _host(ns.coefficients(w))
    Zf = ref.full_basis(ns, WP.size())
    xl, cl = ref.deflate(Zf, vals)
    xb, cb = ref.deflate_bound(Zf, vals)
    assert abs(c[0] - float(cl[0])) <= cb[0]
    assert ns.orthogonalize(w) is w
    got = w.array()
    assert numpy.array_equal(got[:W.size()], vals[:W.size()])   # not streamed
    assert (numpy.abs(got - xl.astype(float)) <= xb).all()
    for x in (fem.Vector(_dev(vals)), _dev(vals)):
        ns.orthogonalize(x)
        data = x.data if isinstance(x, fem.Vector) else x
        assert numpy.array_equal(_host(data), got)
    with pytest.raises(ValueError, match='entries'):
        ns.orthogonalize(device.zeros(WP.size() - 1))
    W1 = fem.VectorFunctionSpace(mesh, 'Lagrange', 1)
    rb = fem.rigid_body_modes(W1)
    u = fem.Function(W1)
    u.set_array(rng.standard_normal(W1.size()))
    rb.orthogonalize(u)
    left = numpy.abs(_host(rb.coefficients(u))).max()
    assert left <= _along(rb.host(), u.array())[1]


# -- shared checks --------------------------------------------------------------------
def _bordered(a, L, bcs, ns):
    A, b = assemble_system(a, L, bcs)
    S, bh = A.to_scipy(), b.get_local()
    Z = ref.full_basis(ns, A.size)
    xs, lam, res = ref.bordered_solve(S, Z, bh)
    assert res < LU_RESIDUAL, res
    return S, bh, Z, xs


def _along(Z, x):
    '''(|Z x|_inf, its rounding bound): what a projection in fp64 leaves
    along the basis -- the entry bounds of the projection summed against |Z|,
    plus the bound of the products that measure it.'''
    xb, cb = ref.deflate_bound(Z, x)
    return numpy.abs(Z.dot(x)).max(), (numpy.abs(Z).dot(xb) + cb).max()


# -- 2. pure Neumann Poisson ----------------------------------------------------------
def _mean_free_source(V):
    '''A Function f of V with assemble(f*dx) = 0 to rounding: the nodal values
    of a smooth g minus their integral mean (the domain has area 1).'''
    c = V.layout.dof_coords
    g = numpy.cos(3.0 * c[:, 0]) * numpy.exp(c[:, 1]) + c[:, 0] ** 2
    f = fem.Function(V)
    f.set_array(g)
    f.set_array(g - ops.integral(f))
    return f


@pytest.mark.parametrize('degree', [1, 2])
def test_pure_neumann_poisson(hip, degree):
    mesh = fem.UnitSquareMesh(8, 6)
    V = fem.FunctionSpace(mesh, 'Lagrange', degree)
    u, v = TrialFunction(V), TestFunction(V)
    a = inner(grad(u), grad(v)) * dx
    f = _mean_free_source(V)
    L = f * v * dx
    ns = fem.constant_nullspace(V)
    S, bh, Z, xs = _bordered(a, L, None, ns)
    uh = fem.Function(V)
    info = solve(a == L, uh, solver_parameters={'krylov_solver': dict(MANY)},
                 nullspace=ns)
    assert info.method == 'cg'
    e = _rel(uh.array(), xs)
    left, bound = _along(Z, uh.array())
    # Z^T b = sum_i b_i / sqrt(n): every b_i carries the roundings of its
    # cell sums (6 cells x 7 points x a few operations: fewer than 256) on
    # terms of at most max|f| times the integral of |phi_i|, whose sum over i
    # is at most 2 (P2 vertex functions change sign) on the unit square
    rounding = 256 * EPS * 2.0 * numpy.abs(f.array()).max() / (
        numpy.sqrt(V.N) * numpy.linalg.norm(bh))
    print('Neumann Poisson P%d: %d its, against the bordered LU %.2e; |Z^T u| '
          '%.2e (bound %.2e); rhs_defect %.2e (rounding %.2e)'
          % (degree, info.iterations, e, left, bound, info.rhs_defect,
             rounding))
    assert e < POISSON_BOUND
    assert left <= bound
    assert info.rhs_defect <= rounding
    # a shifted source: the defect reports the shift, the solve is that of the
    # projected right-hand side
    shift = 0.05
    Ls = (f + fem.Constant(shift)) * v * dx
    _, bs, _, xshift = _bordered(a, Ls, None, ns)
    us = fem.Function(V)
    infos = solve(a == Ls, us,
                  solver_parameters={'krylov_solver': dict(MANY)},
                  nullspace=ns)
    want = numpy.abs(Z.dot(bs)).max() / numpy.linalg.norm(bs)
    print('shifted by %.2f: rhs_defect %.6e, host %.6e; against the bordered '
          'LU %.2e' % (shift, infos.rhs_defect, want, _rel(us.array(), xshift)))
    # (the device's products: within their rounding bound, doubled for the
    # norm and the square root)
    assert abs(infos.rhs_defect - want) <= 2.0 * ref.deflate_bound(Z, bs)[1][0] \
        / numpy.linalg.norm(bs) + 4 * EPS * want
    # roughly the relative shift: the shift over the root mean square of f
    # (load vectors weigh the dofs unevenly: a factor of 5 either way)
    relative = shift / numpy.sqrt(numpy.mean(f.array() ** 2))
    assert 0.2 * relative < infos.rhs_defect < 5.0 * relative
    assert _rel(us.array(), xshift) < POISSON_BOUND


# -- 3. a free elastic body -----------------------------------------------------------
def test_free_elastic_body(hip):
    mesh = fem.UnitSquareMesh(8, 6)
    W = fem.VectorFunctionSpace(mesh, 'Lagrange', 2)
    u, v = TrialFunction(W), TestFunction(W)
    m = MeshFunction('size_t', mesh, 1, 0)
    _Side(lambda x: x[0] < 1e-12).mark(m, 1)
    _Side(lambda x: x[0] > 1.0 - 1e-12).mark(m, 2)
    dsm = Measure('ds', domain=mesh, subdomain_data=m)
    mu, lmbda = 1.0, 1.5
    a = 2.0 * mu * inner(sym(grad(u)), sym(grad(v))) * dx \
        + lmbda * div(u) * div(v) * dx
    # pulled apart at the left and right sides by opposite uniform tractions:
    # neither a net force nor a net moment, self-equilibrated
    pull = fem.Constant((1.0, 0.0))
    L = dot(pull, v) * dsm(2) - dot(pull, v) * dsm(1)
    ns = fem.rigid_body_modes(W)
    S, bh, Z, xs = _bordered(a, L, None, ns)
    uh = fem.Function(W)
    info = solve(a == L, uh, solver_parameters={
        'linear_solver': 'cg', 'krylov_solver': dict(MANY)}, nullspace=ns)
    e = _rel(uh.array(), xs)
    left, bound = _along(Z, uh.array())
    print('free elastic body P2: %s, %d its, against the bordered LU %.2e; '
          '|Z^T u| %.2e (bound %.2e); rhs_defect %.2e'
          % (info.method, info.iterations, e, left, bound, info.rhs_defect))
    assert info.method == 'cg'
    assert e < ELASTIC_BOUND
    assert left <= bound
    # the traction is self-equilibrated: rounding of 3 sums of 2 N terms
    assert info.rhs_defect <= 256 * EPS * numpy.abs(Z).dot(numpy.abs(bh)).max() \
        / numpy.linalg.norm(bh) + 256 * EPS


# -- 4. / 5. enclosed Stokes and Oseen ------------------------------------------------
def _enclosed(nx=8, ny=6):
    '''(WP, conditions): velocity Dirichlet on the whole boundary of the unit
    square, the regularised lid x^2 (1 - x)^2 on the top.'''
    mesh = fem.UnitSquareMesh(nx, ny)
    WP = _space(mesh, 2, 1)
    top = _Side(lambda x: x[1] > 1.0 - 1e-12)
    lid = fem.Expression(('x[0]*x[0]*(1.0 - x[0])*(1.0 - x[0])', '0.0'),
                         degree=4)
    bcs = [fem.DirichletBC(WP.sub(0), fem.Constant((0.0, 0.0)),
                           'on_boundary'),
           fem.DirichletBC(WP.sub(0), lid, top)]
    return mesh, WP, bcs


STOKES_SOLVERS = [
    ('minres jacobi', {'preconditioner': 'jacobi'}),
    ('minres two_level', {'preconditioner': 'two_level'}),
    ('fgmres ilu0', {'linear_solver': 'gmres', 'preconditioner': 'ilu0'}),
    ('fgmres jacobi', {'linear_solver': 'gmres', 'preconditioner': 'jacobi'}),
    ]


def _mixed_solve(WP, a, L, bcs, ns, prm, xs, Z, tag):
    prm = dict(prm)
    prm['krylov_solver'] = dict(LONG, relative_tolerance=1e-12)
    w = fem.Function(WP)
    info = solve(a == L, w, bcs, solver_parameters=prm, nullspace=ns)
    xh = w.array()
    n2 = WP.sub(0).size()
    eu, ep = _rel(xh[:n2], xs[:n2]), _rel(xh[n2:], xs[n2:])
    left, bound = _along(Z, xh)
    print('%-28s %-13s %4d its  u %.2e  p %.2e  |Z^T x| %.2e (bound %.2e)  '
          'rhs_defect %.2e' % (tag, info.method, info.iterations, eu, ep, left,
                               bound, info.rhs_defect))
    assert left <= bound
    return eu, ep, xh, info


def test_enclosed_stokes(hip):
    mesh, WP, bcs = _enclosed()
    W, P = WP.taylor_hood()
    (v, q) = TestFunctions(WP)
    a = _stokes(WP, fem.Constant(0.7))
    f = fem.Expression(('sin(3.0*x[1])', 'x[0]*x[1]'), degree=2)
    L = inner(f, v) * dx
    ns = fem.constant_nullspace(WP)
    S, bh, Z, xs = _bordered(a, L, bcs, ns)
    full = numpy.zeros(WP.size())
    full[W.size():] = ns.host()[0]
    plain = fem.VectorSpaceBasis([full])
    worst_u = worst_p = 0.0
    for tag, prm in STOKES_SOLVERS:
        eu, ep, xh, info = _mixed_solve(WP, a, L, bcs, ns, prm, xs, Z,
                                        'Stokes ' + tag)
        assert info.method == ('minres' if tag.startswith('minres')
                               else 'fgmres+' + prm['preconditioner'])
        # the lid is tangential: the flux through the boundary vanishes and
        # the right-hand side is consistent to rounding
        assert info.rhs_defect <= 256 * EPS * numpy.abs(Z).dot(
            numpy.abs(bh)).max() / numpy.linalg.norm(bh) + 256 * EPS
        worst_u, worst_p = max(worst_u, eu), max(worst_p, ep)
        # full-length vectors without a support: the same bits
        _, _, xh2, info2 = _mixed_solve(WP, a, L, bcs, plain, prm, xs, Z,
                                        '  as full-length vectors')
        assert numpy.array_equal(xh2, xh)
        assert info2.iterations == info.iterations
        assert info2.rhs_defect == info.rhs_defect
    print('enclosed Stokes: worst u %.2e, worst p %.2e' % (worst_u, worst_p))
    assert worst_u < STOKES_U and worst_p < STOKES_P


def test_enclosed_oseen(hip):
    mesh, WP, bcs = _enclosed()
    (v, q) = TestFunctions(WP)
    wu = fem.split(_profile(WP, mesh, 2.0))[0]
    a = _oseen(WP, fem.Constant(0.05), wu)
    f = fem.Expression(('sin(3.0*x[1])', 'x[0]*x[1]'), degree=2)
    L = inner(f, v) * dx
    ns = fem.constant_nullspace(WP)
    S, bh, Z, xs = _bordered(a, L, bcs, ns)
    assert abs(S - S.T).max() > 1e-3
    worst_u = worst_p = 0.0
    for tag, prm in (('fgmres ilu0', {}),
                     ('fgmres jacobi', {'preconditioner': 'jacobi'})):
        eu, ep, _, info = _mixed_solve(WP, a, L, bcs, ns, prm, xs, Z,
                                       'Oseen ' + tag)
        assert info.method.startswith('fgmres+')
        worst_u, worst_p = max(worst_u, eu), max(worst_p, ep)
    assert worst_u < STOKES_U and worst_p < STOKES_P


# -- 6. enclosed Newton -------------------------------------------------------------
NU = 1.0


def _enclosed_navier_stokes():
    '''Steady Navier-Stokes on UnitSquareMesh(8, 8) at Re ~ 1 with the
    divergence-free field u = (x^2, -2 x y), p = x - 1/2 (both in the P2/P1
    space, so the boundary data has no flux to rounding) and velocity
    Dirichlet everywhere.  Returns (WP, bcs, build), build(w) -> (F, J).'''
    mesh = fem.UnitSquareMesh(8, 8)
    WP = _space(mesh, 2, 1)
    ue = fem.Expression(('x[0]*x[0]', '-2.0*x[0]*x[1]'), degree=2)
    f = fem.Expression(('2.0*x[0]*x[0]*x[0] - 2.0*%.17g + 1.0' % NU,
                        '2.0*x[0]*x[0]*x[1]'), degree=3)
    bcs = [fem.DirichletBC(WP.sub(0), ue, 'on_boundary')]

    def build(w):
        (u, p) = fem.split(w)
        (v, q) = TestFunctions(WP)
        (du, dp) = TrialFunctions(WP)
        nu = fem.Constant(NU)
        F = nu * inner(grad(u), grad(v)) * dx + dot(dot(grad(u), u), v) * dx \
            - p * div(v) * dx - q * div(u) * dx - inner(f, v) * dx
        J = nu * inner(grad(du), grad(v)) * dx \
            + dot(dot(grad(du), u), v) * dx + dot(dot(grad(u), du), v) * dx \
            - dp * div(v) * dx - q * div(du) * dx
        return F, J
    return WP, bcs, build


def _start(WP):
    '''Velocity 0, pressure 0.3: a pressure mean the solve has to keep.'''
    w = fem.Function(WP)
    vals = numpy.zeros(WP.size())
    vals[WP.sub(0).size():] = 0.3
    w.set_array(vals)
    return w


def test_enclosed_newton(hip):
    WP, bcs, build = _enclosed_navier_stokes()
    W, P = WP.taylor_hood()
    n2 = W.size()
    ns = fem.constant_nullspace(WP)
    Z = ref.full_basis(ns, WP.size())
    wh = _start(WP)
    Fh, Jh = build(wh)
    iterates, hres, lu = ref.newton(Fh, Jh, wh, bcs, Z)
    assert lu < LU_RESIDUAL, lu
    prm = {'newton_solver': {'krylov_solver': dict(LONG)}}
    w = _start(WP)
    mean0 = Z.dot(w.array())[0]
    F, _ = build(w)
    info = solve(F == 0, w, bcs, solver_parameters=prm, nullspace=ns)
    final = w.array()
    # step by step: every iterate against the host loop's
    ws = _start(WP)
    Fs, _ = build(ws)
    one = {'newton_solver': {'krylov_solver': dict(LONG),
                             'maximum_iterations': 1,
                             'error_on_nonconvergence': False}}
    worst_u = worst_p = 0.0
    for k in range(1, len(iterates)):
        step = solve(Fs == 0, ws, bcs, solver_parameters=one, nullspace=ns)
        assert step.iterations == 1
        xg = ws.array()
        eu = _rel(xg[:n2], iterates[k][:n2])
        ep = _rel(xg[n2:], iterates[k][n2:])
        print('enclosed Newton step %d: %3d its, |F| device %.3e host %.3e; '
              'against the host loop u %.2e p %.2e; rhs_defect %.2e'
              % (k, step.linear_iterations[0], step.residuals[0], hres[k - 1],
                 eu, ep, step.rhs_defect))
        worst_u, worst_p = max(worst_u, eu), max(worst_p, ep)
    eu, ep = _rel(final[:n2], iterates[-1][:n2]), \
        _rel(final[n2:], iterates[-1][n2:])
    worst_u, worst_p = max(worst_u, eu), max(worst_p, ep)
    print('enclosed Newton: worst u %.2e p %.2e; residuals device %s host %s; '
          'rhs_defect %.2e'
          % (worst_u, worst_p, ['%.3e' % r for r in info.residuals],
             ['%.3e' % r for r in hres], info.rhs_defect))
    assert info.converged and info.method == 'fgmres+ilu0'
    assert info.iterations == len(hres) - 1 == len(info.residuals) - 1
    # the same |F| history: the iterates agree to PARITY at the worst, which
    # moves a residual r by about PARITY |F0| -- three digits and a half where
    # r >= 1e-3 |F0|
    for r, h in zip(info.residuals, hres):
        if h >= 1e-3 * hres[0]:
            assert abs(r - h) <= 5e-4 * h, (r, h)
    # the pressure mean of w is the one it started with
    mean1 = Z.dot(final)[0]
    _, cb = ref.deflate_bound(Z, final)
    print('pressure mean (Z^T w): start %.17g, end %.17g'
          % (mean0, mean1))
    assert abs(mean1 - mean0) <= (info.iterations + 1) * (
        cb[0] + _along(Z, final)[1])
    # against the exact fields: p up to its mean
    xu, xp = W.layout.dof_coords, P.layout.dof_coords
    exact_u = numpy.concatenate([xu[:, 0] ** 2, -2.0 * xu[:, 0] * xu[:, 1]])
    pe = xp[:, 0] - 0.5
    ph = final[n2:]
    print('against the exact fields: u %.2e, p - mean %.2e'
          % (_rel(final[:n2], exact_u),
             _rel(ph - ph.mean(), pe - pe.mean())))
    assert worst_u < NEWTON_U and worst_p < NEWTON_P


# -- 7. refusals ----------------------------------------------------------------------
def test_refusals(hip, monkeypatch):
    mesh = fem.UnitSquareMesh(8, 6)
    V = fem.FunctionSpace(mesh, 'Lagrange', 1)
    V2 = fem.FunctionSpace(mesh, 'Lagrange', 2)
    u, v = TrialFunction(V), TestFunction(V)
    a = inner(grad(u), grad(v)) * dx
    L = _mean_free_source(V) * v * dx
    ns = fem.constant_nullspace(V)
    # (a Function's zero fill is a launch: both are made before the count)
    uh, un = fem.Function(V), fem.Function(V)
    before = _hip.launch_count()
    with pytest.raises(ValueError, match='not orthonormal'):
        solve(a == L, uh, nullspace=fem.VectorSpaceBasis([numpy.ones(V.N)]))
    with pytest.raises(ValueError, match='another space'):
        solve(a == L, uh, nullspace=fem.constant_nullspace(V2))
    with pytest.raises(ValueError, match='wrong length'):
        solve(a == L, uh, nullspace=fem.VectorSpaceBasis(
            [numpy.full(V2.N, V2.N ** -0.5)]))
    bc = fem.DirichletBC(V, fem.Constant(0.0), 'on_boundary')
    with pytest.raises(ValueError, match='Dirichlet dof'):
        solve(a == L, uh, [bc], nullspace=ns)
    with pytest.raises(TypeError, match='VectorSpaceBasis'):
        solve(a == L, uh, nullspace=[numpy.ones(V.N)])
    # the ILU(0) routes, and any method but CG
    conv = a + dot(fem.Constant((8.0, -3.0)), grad(u)) * v * dx
    with pytest.raises(NotImplementedError, match='ILU'):
        solve(conv == L, uh, nullspace=ns)
    with pytest.raises(NotImplementedError, match='CG route'):
        solve(a == L, uh, solver_parameters={'linear_solver': 'bicgstab'},
              nullspace=ns)
    # Newton's method on scalar and vector spaces
    Fn = inner(grad(un), grad(v)) * dx + un * un * un * v * dx - v * dx
    with pytest.raises(NotImplementedError, match='Newton'):
        solve(Fn == 0, un, nullspace=ns)
    assert _hip.launch_count() == before
    # a vector that is not in the nullspace: refused by the |A z| check
    # (after the assembly), let through by nullspace_check=False
    am = a + u * v * dx
    with pytest.raises(ValueError, match='not in the nullspace'):
        solve(am == L, uh, nullspace=ns)
    for check in (False, 1.0e6):
        info = solve(am == L, uh, nullspace=ns,
                     solver_parameters={'nullspace_check': check})
        assert info.method == 'cg' and info.rhs_defect is not None
    # ... and on a Taylor-Hood space
    _, WP, bcs = _enclosed()
    (up, pp), (vp, qp) = TrialFunctions(WP), TestFunctions(WP)
    nsp = fem.constant_nullspace(WP)
    sa = _stokes(WP, fem.Constant(0.7))
    sL = inner(fem.Constant((0.0, 1.0)), vp) * dx
    w = fem.Function(WP)
    P = WP.sub(1)
    pin = FixedDofsBC(P, [0], [0.0])
    for prm in ({}, {'linear_solver': 'gmres'}):
        with pytest.raises(ValueError, match='Dirichlet dof'):
            solve(sa == sL, w, bcs + [pin], solver_parameters=prm,
                  nullspace=nsp)
        with pytest.raises(ValueError, match='another space'):
            solve(sa == sL, w, bcs, solver_parameters=prm, nullspace=ns)
        # with a p*q term the pressure constant is no null vector
        with pytest.raises(ValueError, match='not in the nullspace'):
            solve(sa - 0.1 * pp * qp * dx == sL, w, bcs,
                  solver_parameters=prm, nullspace=nsp)
    WPn, bcn, build = _enclosed_navier_stokes()
    wn = _start(WPn)
    with pytest.raises(ValueError, match='not orthonormal'):
        solve(build(wn)[0] == 0, wn, bcn, nullspace=fem.VectorSpaceBasis(
            [numpy.ones(WPn.sub(1).N)],
            support=(WPn.sub(0).size(), WPn.sub(1).N)))
    # strips
    from flow_amd import parallel
    monkeypatch.setattr(parallel, 'active', lambda nrows=None: True)
    with pytest.raises(NotImplementedError, match='strips'):
        solve(a == L, uh, nullspace=ns)


# -- 8. nullspace=None ----------------------------------------------------------------
def test_none_changes_nothing(hip):
    def twice(run):
        '''run(kwargs) -> (field, info): without the keyword and with None.'''
        x0, i0 = run({})
        x1, i1 = run({'nullspace': None})
        assert numpy.array_equal(x0, x1)
        return i0, i1

    # the CG route
    mesh = fem.UnitSquareMesh(8, 6)
    V = fem.FunctionSpace(mesh, 'Lagrange', 2)
    u, v = TrialFunction(V), TestFunction(V)
    bc = fem.DirichletBC(V, fem.Constant(0.5), 'on_boundary')

    def cg(kw):
        uh = fem.Function(V)
        info = solve(inner(grad(u), grad(v)) * dx
                     == fem.Constant(1.0) * v * dx, uh, [bc], **kw)
        return uh.array(), info

    i0, i1 = twice(cg)
    assert (i0.method, i0.iterations, i0.residual) == \
        (i1.method, i1.iterations, i1.residual) and i1.rhs_defect is None
    # MINRES and FGMRES
    WP, cases = _cases('square')
    sa, sL, sbcs, _ = cases['d Stokes by gmres']
    for prm, method in (({}, 'minres'),
                        ({'linear_solver': 'gmres'}, 'fgmres+ilu0')):
        def mixed_solve(kw):
            w = fem.Function(WP)
            info = solve(sa == sL, w, sbcs, solver_parameters=prm, **kw)
            return w.array(), info

        i0, i1 = twice(mixed_solve)
        assert i0.method == i1.method == method
        assert (i0.iterations, i0.residual) == (i1.iterations, i1.residual)
        assert i1.rhs_defect is None
    # Newton's method, with a corner pin
    WPn, bcn, build = _enclosed_navier_stokes()
    pin = FixedDofsBC(WPn.sub(1), [0], [0.0])

    def newton(kw):
        w = fem.Function(WPn)
        info = solve(build(w)[0] == 0, w, bcn + [pin], solver_parameters={
            'newton_solver': {'krylov_solver': dict(LONG)}}, **kw)
        return w.array(), info

    i0, i1 = twice(newton)
    assert i0.residuals == i1.residuals
    assert i0.linear_iterations == i1.linear_iterations
    assert i1.rhs_defect is None
