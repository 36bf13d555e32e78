# -*- coding: utf-8 -*-
'''
The non-symmetric mixed solve on the GPU (fem.mixed_gmres; flow_amd/fem/
mixed.py, csrc/mixed_kernels.hip): the one-launch block product
MixedMatrix.apply_fused bit for bit against the composed MixedMatrix.apply for
every pattern of present blocks and against the host product, flexible GMRES
with the block-triangular preconditioner against sparse LU on Oseen, +q*div(u),
Brinkman / traction and forced-GMRES Stokes problems, the sign of the Schur
diagonal, a Picard loop on Kovasznay's flow, and fgmres alone on a scalar
matrix.
'''
import numpy
import pytest
import scipy.sparse.linalg as spla
import torch

from flow_amd import fem, _hip, device
from flow_amd.fem import (
    TestFunction, TrialFunction, TestFunctions, TrialFunctions, assemble,
    assemble_system, solve, dx, Measure, MeshFunction, SpatialCoordinate, dot,
    inner, grad, div, sym,
    )
from flow_amd.fem import ops, mixed
from flow_amd.fem.bcs import FixedDofsBC

pytestmark = pytest.mark.gpu

# the relative bound of tests/test_mixed_forms_gpu.py for the composed product
TOL = 1e-12
# field parity (README): no solve may differ by more
PARITY = 1e-7
EPS = 2.0 ** -52


@pytest.fixture(autouse=True)
def _switches_on():
    with fem.mixed_arguments(True), fem.vector_arguments(True), \
            fem.facet_arguments(True), fem.cell_subdomains(True), \
            fem.mixed_gmres(True):
        yield


class _Side(fem.SubDomain):
    def __init__(self, test):
        fem.SubDomain.__init__(self)
        self.test = test

    def inside(self, x, on_boundary):
        return on_boundary & self.test(x)


class _Cells(fem.SubDomain):
    def __init__(self, test):
        fem.SubDomain.__init__(self)
        self.test = test

    def inside(self, x, on_boundary):
        return self.test(x)


def _meshes():
    return [fem.UnitSquareMesh(12, 9), fem.karman_channel(60, 14, fitted=True)]


def _space(mesh, kv, kp):
    return fem.FunctionSpace(
        mesh, fem.VectorElement('Lagrange', 'triangle', kv)
        * fem.FiniteElement('Lagrange', 'triangle', kp))


PAIRS = [(2, 1), (1, 1)]


def _box(mesh):
    return mesh.points.min(axis=0), mesh.points.max(axis=0)


def _profile(WP, mesh, scale=1.0):
    '''A mixed Function whose velocity is the parabolic profile between the
    lower and the upper wall (pressure 0).'''
    (x0, y0), (x1, y1) = _box(mesh)
    W = WP.sub(0)
    y = W.layout.dof_coords[:, 1]
    ux = scale * 4.0 * (y - y0) * (y1 - y) / (y1 - y0) ** 2
    w = fem.Function(WP)
    vals = numpy.zeros(WP.size())
    vals[:W.N] = ux
    w.set_array(vals)
    return w


def _stokes(WP, mu):
    (u, p) = TrialFunctions(WP)
    (v, q) = TestFunctions(WP)
    return mu * inner(grad(u), grad(v)) * dx - p * div(v) * dx \
        - q * div(u) * dx


def _oseen(WP, nu, wu, sign=-1.0):
    (u, p) = TrialFunctions(WP)
    (v, q) = TestFunctions(WP)
    return nu * inner(grad(u), grad(v)) * dx \
        + dot(dot(grad(u), wu), v) * dx - p * div(v) * dx \
        + sign * q * div(u) * dx


def _rel(got, want):
    return numpy.abs(got - want).max() / numpy.abs(want).max()


def _dev(a):
    return device.to_device(numpy.ascontiguousarray(a, dtype=numpy.float64))


def _host(t):
    return t.cpu().numpy().copy()


def _vectors(n, seed, count=3):
    rng = numpy.random.RandomState(seed)
    return [rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 3, n)
            for _ in range(count)]


def _both_products(A, xs):
    '''(apply, apply_fused) of the host vector xs, outputs preset to NaN.'''
    x = _dev(xs)
    out = []
    for fn in (A.apply, A.apply_fused):
        y = torch.full((A.size,), float('nan'), dtype=torch.float64,
                       device=x.device)
        out.append(_host(fn(x, y)))
    return out


# -- 4. bits ----------------------------------------------------------------------
def test_apply_fused_bits_all_blocks_and_missing_blocks(hip):
    for mesh in _meshes():
        x = SpatialCoordinate(mesh)
        for kv, kp in PAIRS:
            WP = _space(mesh, kv, kp)
            (u, p), (v, q) = TrialFunctions(WP), TestFunctions(WP)
            wu = fem.split(_profile(WP, mesh, 1.5))[0]
            nu, c = 1.0 + x[0], 1.0 + x[0] * x[1]
            a = 2.0 * nu * inner(sym(grad(u)), sym(grad(v))) * dx \
                + dot(u, v) * dx + dot(dot(grad(u), wu), v) * dx \
                - p * div(v) * dx - q * div(u) * dx - 0.1 * c * p * q * dx
            A = assemble(a)
            assert len(A.blocks()) == 6
            tag = '%d cells P%d/P%d' % (mesh.num_cells(), kv, kp)
            s = A.fused()
            print('%s: %d velocity tiles, %d pressure tiles'
                  % (tag, s.nvtiles, s.nptiles))
            subsets = {
                'all blocks': A,
                'no pp': mixed.MixedMatrix(WP, A.uu, None, A.up, A.pu),
                'no up': mixed.MixedMatrix(WP, A.uu, A.pp, None, A.pu),
                'no pu': mixed.MixedMatrix(WP, A.uu, A.pp, A.up, None),
                'no up1, no pu0': mixed.MixedMatrix(
                    WP, A.uu, A.pp, [A.up[0], None], [None, A.pu[1]]),
                'only uu': mixed.MixedMatrix(WP, A.uu),
                'only the couplings': mixed.MixedMatrix(WP, None, None, A.up,
                                                        A.pu),
                'only pu1': mixed.MixedMatrix(WP, None, None, None,
                                              [None, A.pu[1]]),
                }
            for name, B in subsets.items():
                for xs in _vectors(A.size, 5):
                    want, got = _both_products(B, xs)
                    assert not numpy.isnan(want).any()
                    bad = numpy.nonzero(~((got == want) | (
                        numpy.isnan(got) & numpy.isnan(want))))[0]
                    assert numpy.array_equal(got, want), (
                        tag, name, len(bad), bad[:8], got[bad[:4]],
                        want[bad[:4]])
                    # two calls give equal bits
                    assert numpy.array_equal(_both_products(B, xs)[1], got)
            want, got = _both_products(subsets['only uu'], _vectors(A.size, 6)[0])
            assert (got[2 * WP.sub(0).N:] == 0.0).all()
            # x is y: refused, nothing launched
            xd = _dev(_vectors(A.size, 7)[0])
            before = _hip.launch_count()
            with pytest.raises(ValueError, match='overlaps'):
                A.apply_fused(xd, xd)
            with pytest.raises(ValueError, match='overlaps'):
                buf = torch.zeros(A.size + 8, dtype=torch.float64,
                                  device=xd.device)
                A.apply_fused(buf[:A.size], buf[8:])
            assert _hip.launch_count() == before


# -- 5. against the host ----------------------------------------------------------
def test_apply_fused_against_scipy(hip):
    for mesh in _meshes():
        x = SpatialCoordinate(mesh)
        for kv, kp in PAIRS:
            WP = _space(mesh, kv, kp)
            (u, p), (v, q) = TrialFunctions(WP), TestFunctions(WP)
            wu = fem.split(_profile(WP, mesh))[0]
            a = _oseen(WP, fem.Constant(0.7), wu) + dot(u, v) * dx \
                - (1.0 + x[0]) * p * q * dx
            A = assemble(a)
            S = A.to_scipy()
            for xs in _vectors(A.size, 8, 2):
                got = _both_products(A, xs)[1]
                e = _rel(got, S @ xs)
                print('apply_fused vs scipy, %d cells P%d/P%d: %.2e'
                      % (mesh.num_cells(), kv, kp, e))
                assert e < TOL


# -- 6. solves --------------------------------------------------------------------
# Measured on an MI355X on the first run of these tests: max-norm difference
# from scipy's sparse LU of the same assemble_system, relative to max|u| and
# max|p|, after FGMRES at relative 1e-12 on the true residual; u, p
# (iterations), ilu0 then jacobi.  UnitSquareMesh(8, 6) P2/P1 on the defaults
# (restart 30; jacobi with LONG below), the fitted channel (60, 14) with LONG:
#   square  a Oseen             5.7e-12 3.6e-11 (74)    9.1e-12 1.3e-11 (128)
#           a, preconditioner_form      1.2e-11 2.7e-11 (103)
#           b Stokes + 2 q div u 7.0e-12 1.2e-11 (82)   3.7e-12 6.5e-12 (145)
#           c Brinkman, traction 1.1e-11 1.4e-11 (69)   1.4e-11 1.5e-11 (123)
#           d Stokes by gmres   7.0e-12 1.2e-11 (82)    3.7e-12 6.5e-12 (145)
#   channel a Oseen             3.1e-11 2.1e-11 (226)   4.5e-11 2.0e-11 (1114)
#           a, preconditioner_form      5.4e-11 4.0e-11 (208)
#           b Stokes + 2 q div u 1.4e-11 8.3e-12 (225)  5.7e-12 2.7e-12 (1139)
#           c Brinkman, traction 3.1e-11 1.3e-11 (225)  4.9e-11 2.0e-11 (1109)
#           d Stokes by gmres   1.4e-11 8.5e-12 (225)   5.6e-12 2.4e-12 (1139)
#   +q*div(u) against -q*div(u): the same bits (rows and Schur diagonal change
#   sign together), 74 / 226 iterations
#   Picard on Kovasznay's flow, 30 steps, each against the host loop's step:
#   u <= 2.24e-9, p <= 3.61e-8 (step 17, 45 iterations; 92 .. 133 iterations
#   while the increment is above 1e-7: the pressure pinned at one corner
#   vertex is a weakly determined mode, so a residual of 1e-12 |b| leaves more
#   in p there than in the other problems)
# The bounds are 10x the largest measured figure of their kind, capped by the
# field-parity bound: 2.24e-8 for u, and the cap for p (10 x 3.61e-8 is above
# it).
SOLVE_BOUND_U = min(PARITY, 10 * 2.24e-9)
SOLVE_BOUND_P = min(PARITY, 10 * 3.61e-8)

NU = 0.05


def _problem(which):
    '''mesh, WP, Dirichlet conditions (inflow profile on the left, no slip on
    everything but the left and right sides), a pressure pin on the right
    side, ds / dx measures (facets 2: the right side; cells 1: the left
    half), and the Poiseuille profile as a mixed Function.'''
    mesh = fem.UnitSquareMesh(8, 6) if which == 'square' \
        else fem.karman_channel(60, 14, fitted=True)
    WP = _space(mesh, 2, 1)
    (x0, y0), (x1, y1) = _box(mesh)
    tol = 1e-10 * (x1 - x0)
    left = _Side(lambda x: x[0] < x0 + tol)
    right = _Side(lambda x: x[0] > x1 - tol)
    walls = _Side(lambda x: (x[0] > x0 + tol) & (x[0] < x1 - tol))
    prof = '4.0*(x[1] - (%.17g))*((%.17g) - x[1])/%.17g' % (
        y0, y1, (y1 - y0) ** 2)
    bcs = [fem.DirichletBC(WP.sub(0), fem.Expression((prof, '0.0'), degree=2),
                           left),
           fem.DirichletBC(WP.sub(0), fem.Constant((0.0, 0.0)), walls)]
    pin = fem.DirichletBC(WP.sub(1), fem.Constant(0.0), right)
    facets = MeshFunction('size_t', mesh, 1)
    facets.set_all(0)
    right.mark(facets, 2)
    cellm = MeshFunction('size_t', mesh, 2)
    cellm.set_all(0)
    _Cells(lambda x: x[0] < 0.5 * (x0 + x1)).mark(cellm, 1)
    dsm = Measure('ds', domain=mesh, subdomain_data=facets)
    dxm = Measure('dx', domain=mesh, subdomain_data=cellm)
    return mesh, WP, bcs, pin, dsm, dxm, _profile(WP, mesh)


def _cases(which):
    '''name -> (a, L, bcs, preconditioner form or None)'''
    mesh, WP, bcs, pin, dsm, dxm, w0 = _problem(which)
    (u, p), (v, q) = TrialFunctions(WP), TestFunctions(WP)
    wu = fem.split(w0)[0]
    nu = fem.Constant(NU)
    f = fem.Expression(('sin(3.0*x[1])', 'x[0]*x[1]'), degree=2)
    L = inner(f, v) * dx
    oseen = _oseen(WP, nu, wu)
    prec = nu * inner(grad(u), grad(v)) * dx - (1.0 / NU) * p * q * dx
    return WP, {
        'a Oseen': (oseen, L, bcs, prec),
        'b Stokes + 2 q div u': (
            _stokes(WP, fem.Constant(0.7)) + 2.0 * q * div(u) * dx, L,
            bcs + [pin], None),
        'c Oseen, Brinkman dx(1), traction ds(2)': (
            oseen + 3.0 * dot(u, v) * dxm(1),
            L + dot(fem.Constant((-0.5, 0.25)), v) * dsm(2), bcs, None),
        'd Stokes by gmres': (_stokes(WP, fem.Constant(0.7)), L, bcs + [pin],
                              None),
        }


def _check_solve(WP, a, L, bcs, prm, tag):
    '''One solve against sparse LU of the same system: prints and returns the
    two figures; asserts the stopping rule on the host and the method.'''
    A, b = assemble_system(a, L, bcs)
    S = A.to_scipy()
    bh = b.get_local()
    xs = spla.spsolve(S.tocsc(), bh)
    w = fem.Function(WP)
    info = solve(a == L, w, bcs, solver_parameters=prm)
    xh = w.array()
    n2 = WP.sub(0).size()
    eu, ep = _rel(xh[:n2], xs[:n2]), _rel(xh[n2:], xs[n2:])
    ks = prm.get('krylov_solver', {})
    tol = max(ks.get('relative_tolerance', 1e-12) * numpy.linalg.norm(bh),
              ks.get('absolute_tolerance', 0.0))
    res = numpy.linalg.norm(bh - S @ xh)
    # (the host's residual differs from the device's by the rounding of one
    # product: <= (row length + 2) eps |A| |x| per row, TOL's argument)
    slack = numpy.linalg.norm(
        (numpy.diff(S.indptr) + 2) * EPS * (abs(S) @ numpy.abs(xh)
                                            + numpy.abs(bh)))
    print('%-62s %-13s %4d its  u %.2e  p %.2e  |r| %.2e (host %.2e, tol '
          '%.2e)' % (tag, info.method, info.iterations, eu, ep, info.residual,
                     res, tol))
    assert info.method == 'fgmres+' + prm.get('preconditioner', 'ilu0')
    assert info.residual <= tol
    assert res <= tol + slack
    assert info.iterations <= ks.get('maximum_iterations', 1000)
    return eu, ep, xh, info


# GMRES(30) stagnates on the stretched cells of the fitted channel and under
# Jacobi: those solves keep a longer basis (the square with ILU(0) runs on the
# defaults)
LONG = {'restart': 400, 'maximum_iterations': 4000}
JACOBI = {'preconditioner': 'jacobi', 'krylov_solver': dict(LONG)}


@pytest.mark.parametrize('which', ['square', 'channel'])
def test_solves_against_sparse_lu(hip, which):
    WP, cases = _cases(which)
    worst_u = worst_p = 0.0
    for name, (a, L, bcs, prec) in cases.items():
        prms = [{}, dict(JACOBI)]
        if prec is not None:
            prms.append({'preconditioner_form': prec})
        for prm in prms:
            prm = dict(prm)
            if which == 'channel':
                prm['krylov_solver'] = dict(LONG)
            if name.startswith('d'):
                prm['linear_solver'] = 'gmres'
            tag = '%s %s %s' % (which, name, 'form' if
                                'preconditioner_form' in prm else '')
            eu, ep = _check_solve(WP, a, L, bcs, prm, tag)[:2]
            worst_u, worst_p = max(worst_u, eu), max(worst_p, ep)
    print('%s: worst u %.2e, worst p %.2e' % (which, worst_u, worst_p))
    assert worst_u < SOLVE_BOUND_U and worst_p < SOLVE_BOUND_P


def test_refusals_and_switch_off(hip):
    WP, cases = _cases('square')
    a, L, bcs, _ = cases['a Oseen']
    w = fem.Function(WP)
    with pytest.raises(ValueError, match="'ilu0' or 'jacobi'"):
        solve(a == L, w, bcs,
              solver_parameters={'preconditioner': 'two_level'})
    with pytest.raises(ValueError, match="'ilu0' or 'jacobi'"):
        mixed.BlockTriangularPreconditioner(assemble(a), 'two_level')
    (u, p), (v, q) = TrialFunctions(WP), TestFunctions(WP)
    with pytest.raises(ValueError, match='no velocity-velocity block'):
        solve(-p * div(v) * dx + q * div(u) * dx + p * q * dx == L, w, [])
    with fem.mixed_gmres(False):
        with pytest.raises(NotImplementedError, match='non-symmetric'):
            solve(a == L, w, bcs)
        # a symmetric form keeps MINRES, whatever 'linear_solver' says
        sa, sL, sbcs, _ = cases['d Stokes by gmres']
        info = solve(sa == sL, fem.Function(WP), sbcs,
                     solver_parameters={'linear_solver': 'gmres'})
        assert info.method == 'minres'
    # the default of a symmetric form stays MINRES with the switch on
    sa, sL, sbcs, _ = cases['d Stokes by gmres']
    assert solve(sa == sL, fem.Function(WP), sbcs).method == 'minres'


# -- 7. sign ----------------------------------------------------------------------
@pytest.mark.parametrize('which', ['square', 'channel'])
def test_sign_of_the_divergence_row(hip, which):
    mesh, WP, bcs, pin, dsm, dxm, w0 = _problem(which)
    (u, p), (v, q) = TrialFunctions(WP), TestFunctions(WP)
    wu = fem.split(w0)[0]
    f = fem.Expression(('sin(3.0*x[1])', 'x[0]*x[1]'), degree=2)
    L = inner(f, v) * dx
    fields, its = [], []
    for sign in (-1.0, 1.0):
        a = _oseen(WP, fem.Constant(NU), wu, sign)
        A, _ = assemble_system(a, L, bcs)
        d = _host(mixed._signed_schur_diagonal(A, None))
        assert (sign * d[d != 1.0] > 0.0).all() and (d != 1.0).any()
        prm = {'krylov_solver': dict(LONG)} if which == 'channel' else {}
        _, _, xh, info = _check_solve(WP, a, L, bcs, prm,
                                      '%s sign %+d' % (which, sign))
        its.append(info.iterations)
        fields.append(xh)
    n2 = WP.sub(0).size()
    eu = _rel(fields[1][:n2], fields[0][:n2])
    ep = _rel(fields[1][n2:], fields[0][n2:])
    print('%s: +q div u against -q div u: u %.2e p %.2e (%d and %d its)'
          % (which, eu, ep, its[1], its[0]))
    assert eu < SOLVE_BOUND_U and ep < SOLVE_BOUND_P


# -- 8. Picard ----------------------------------------------------------------------
# chosen on an MI355X: the increment of the GPU loop falls by a factor of 2 to
# 10 per step, is 5.3e-11 at step 24 and exactly 0 (FGMRES takes no iteration)
# from step 25 on
PICARD_STEPS = 26


def test_picard_kovasznay(hip):
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
    exact_p = pe(xp)
    (v, q) = TestFunctions(WP)
    L = inner(fem.Constant((0.0, 0.0)), v) * dx
    n2 = W.size()

    def form(w_old):
        return _oseen(WP, fem.Constant(1.0 / re), fem.split(w_old)[0])

    gpu_old, host_old = fem.Function(WP), fem.Function(WP)
    a_gpu, a_host = form(gpu_old), form(host_old)
    w = fem.Function(WP)
    worst_u = worst_p = 0.0
    for step in range(PICARD_STEPS):
        info = solve(a_gpu == L, w, bcs,
                     solver_parameters={'krylov_solver': dict(LONG)})
        A, b = assemble_system(a_host, L, bcs)
        xs = spla.spsolve(A.to_scipy().tocsc(), b.get_local())
        xg = w.array()
        inc = numpy.abs(xg - gpu_old.array()).max()
        eu, ep = _rel(xg[:n2], xs[:n2]), _rel(xg[n2:], xs[n2:])
        print('Picard %2d: %3d its, increment %.2e, against the host loop u '
              '%.2e p %.2e; against the exact fields u %.2e p %.2e'
              % (step + 1, info.iterations, inc, eu, ep,
                 _rel(xg[:n2], exact_u), _rel(xg[n2:], exact_p)))
        worst_u, worst_p = max(worst_u, eu), max(worst_p, ep)
        gpu_old.set_array(xg)
        host_old.set_array(xs)
    assert worst_u < SOLVE_BOUND_U and worst_p < SOLVE_BOUND_P


# -- 9. fgmres alone ------------------------------------------------------------------
# measured on an MI355X, relative max-norm difference from sparse LU: identity
# 4.74e-12, Jacobi 2.52e-12 (79 iterations each); 10x, capped by parity
FGMRES_BOUND = min(PARITY, 10 * 4.74e-12)


def test_fgmres_on_a_scalar_matrix(hip):
    mesh = fem.UnitSquareMesh(12, 9)
    V = fem.FunctionSpace(mesh, 'Lagrange', 1)
    u, v = TrialFunction(V), TestFunction(V)
    x = SpatialCoordinate(mesh)
    a = inner(grad(u), grad(v)) * dx \
        + dot(fem.Constant((8.0, -3.0)), grad(u)) * v * dx
    L = (1.0 + x[0]) * v * dx
    bc = fem.DirichletBC(V, fem.Constant(0.5), 'on_boundary')
    A, b = assemble_system(a, L, [bc])
    S = A.to_scipy()
    assert abs(S - S.T).max() > 1e-3
    bh = b.get_local()
    xs = spla.spsolve(S.tocsc(), bh)
    dinv = A.diag_inv()
    tol = 1e-12 * numpy.linalg.norm(bh)
    for name, prec in (('identity', lambda r, z: ops.copy(z, r)),
                       ('jacobi', lambda r, z: ops.vmul(r, dinv, z))):
        xd = device.zeros(V.size())
        its, res = mixed.fgmres(A.apply, prec, b.data, xd, 1e-12,
                                maxit=20000, restart=5)
        e = _rel(_host(xd), xs)
        print('fgmres(5) %-8s: %5d its, |r| %.2e (tol %.2e), against LU %.2e'
              % (name, its, res, tol, e))
        assert its > 5            # restarts happened
        assert res <= tol
        assert e < FGMRES_BOUND
        # the same call gives the same bits
        xd2 = device.zeros(V.size())
        assert mixed.fgmres(A.apply, prec, b.data, xd2, 1e-12, maxit=20000,
                            restart=5) == (its, res)
        assert numpy.array_equal(_host(xd2), _host(xd))
        with pytest.raises(_hip.NotConverged):
            mixed.fgmres(A.apply, prec, b.data, device.zeros(V.size()),
                         1e-12, maxit=3, restart=5)
