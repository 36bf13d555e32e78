# -*- coding: utf-8 -*-
'''
conditional, max_value / min_value / sign / tanh, the cell geometry operands
and the SUPG tau operand on the HIP path: forms of rank 0, 1 and 2 against the
numpy evaluator of tests/conditional_reference.py at the same rule, geometry
sums against the mesh arrays, a singular untaken branch, determinism,
flow_supg_tau against the tau of the heat assembly, the reference's SUPG heat
operator from its own form text against the dedicated kernels, and a Newton
solve with a clipped coefficient against the host Newton.
'''
import numpy
import pytest

from flow_amd import fem, stabilization
from flow_amd.heat import Heat
from flow_amd.fem import (
    TestFunction, TrialFunction, dx, ds, dot, inner, grad, sqrt, exp,
    SpatialCoordinate, lhs, rhs, assemble, assemble_system, Probes,
    conditional, lt, gt, ge, eq, ne, And, Or, Not, max_value, min_value, sign,
    tanh,
    CellVolume, Circumradius, CellDiameter,
    )

import conditional_reference as cref
import point_reference as pref

pytestmark = pytest.mark.gpu


def _meshes():
    return [fem.UnitSquareMesh(12, 9),
            fem.karman_channel(60, 14, fitted=True),
            fem.karman_channel_graded(lcar=1.0e-2)]


def _field(V, funcs):
    u = fem.Function(V)
    xy = V.layout.dof_coords
    u.set_array(numpy.concatenate([f(xy[:, 0], xy[:, 1]) for f in funcs]))
    return u


def _err(got, ref, what=''):
    '''max entrywise error relative to max|entry| (printed: the measured
    figure is part of the record).'''
    got = got.toarray() if hasattr(got, 'toarray') else numpy.asarray(got)
    ref = ref.toarray() if hasattr(ref, 'toarray') else numpy.asarray(ref)
    e = numpy.abs(got - ref).max() / numpy.abs(ref).max()
    print('%-52s %.2e' % (what, e))
    return e


def _vals(A):
    return A.plane(0).cpu().numpy()


def _operands(mesh):
    P2 = fem.FunctionSpace(mesh, 'CG', 2)
    W = fem.VectorFunctionSpace(mesh, 'CG', 2)
    th = _field(P2, [lambda x, y: 0.5 + numpy.sin(3 * x) * y])
    w = _field(W, [lambda x, y: 1.0 + x * y, lambda x, y: numpy.cos(2 * y) - x])
    return th, w


def _coefficients(mesh):
    '''Scalar coefficients that use every new node; both sides of every
    switch occur on each mesh.'''
    th, w = _operands(mesh)
    X = SpatialCoordinate(mesh)
    h, R, T = CellDiameter(mesh), Circumradius(mesh), CellVolume(mesh)
    xm = float(mesh.points[:, 0].mean())
    c1 = conditional(And(gt(th, 0.5), Not(lt(X[0], 0.25 * xm))),
                     tanh(3.0 * th) + h, max_value(th, 0.2) * X[1] + R)
    c2 = min_value(th * th, 0.6) + sign(th - 0.5) * sqrt(T) \
        + conditional(Or(lt(X[0], xm), ge(h, 10.0)), exp(-th), R / h)
    c3 = max_value(0.0, 0.3 * h * sqrt(dot(w, w)) - 0.01) + tanh(0.05 * X[0])
    return th, w, c1, c2, c3


def test_ranks_against_the_evaluator(hip):
    for m, mesh in enumerate(_meshes()):
        th, w, c1, c2, c3 = _coefficients(mesh)
        tag = 'mesh %d ' % m
        for k, c in enumerate((c1, c2, c3)):
            form = c * dx(mesh)
            assert _err(assemble(form), cref.functional(form),
                        tag + 'functional c%d' % (k + 1)) < 1e-12
        # (on the boundary y = 0 th is 0.5 up to rounding: the facet
        # integrand switches at 0.37, not at c1's and c2's 0.5)
        h = CellDiameter(mesh)
        facet = conditional(gt(th, 0.37), tanh(3.0 * th) + h,
                            max_value(th, 0.2) * Circumradius(mesh)) * c3 \
            + min_value(th, 0.6) * h + sign(th - 0.37) * CellVolume(mesh)
        form = facet * ds(mesh) + c2 * dx(mesh)
        assert _err(assemble(form), cref.functional(form),
                    tag + 'ds + dx functional') < 1e-12
        for V in [fem.FunctionSpace(mesh, 'CG', k) for k in (1, 2)]:
            u, v = TrialFunction(V), TestFunction(V)
            tg = tag + 'P%d ' % V.degree
            L = (c1 * v + c3 * dot(w, grad(v))
                 + conditional(gt(th, 0.5), v.dx(0), th * v)) * dx
            assert _err(assemble(L).get_local(), cref.vector(L),
                        tg + 'vector') < 1e-12
            a = (c3 * inner(grad(u), grad(v)) + c2 * u * v
                 + conditional(gt(th, 0.5), dot(w, grad(u)) * v,
                               u * dot(w, grad(v)))) * dx
            assert _err(assemble(a).to_scipy(), cref.matrix(a),
                        tg + 'matrix') < 1e-12


def test_point_evaluation(hip):
    for m, mesh in enumerate(_meshes()[:2]):
        th, w, c1, c2, c3 = _coefficients(mesh)
        pts = pref.random_points(mesh, 300, seed=4, margin=0.0)
        probes = Probes(mesh, pts)
        f = probes.found
        assert f.sum() > 100
        for k, c in enumerate((c1, c2, c3)):
            want = cref.point_values(c, mesh, pts[f], probes.cells[f])[0]
            assert _err(probes(c)[f], want,
                        'mesh %d c%d at points' % (m, k + 1)) < 1e-12


def test_geometry_sums(hip):
    for m, mesh in enumerate(_meshes()):
        q = cref.cell_quantities(mesh)
        area = q[:, 0]
        nc = mesh.num_cells()
        tag = 'mesh %d ' % m
        assert _err(assemble(CellVolume(mesh) * dx), (area**2).sum(),
                    tag + 'sum |T|^2') < 1e-12
        assert _err(assemble(1 / CellVolume(mesh) * dx), float(nc),
                    tag + 'number of cells') < 1e-12
        assert _err(assemble(Circumradius(mesh) * dx(mesh)),
                    (q[:, 1] * area).sum(), tag + 'sum R |T|') < 1e-12
        assert _err(assemble(CellDiameter(mesh) * dx(mesh)),
                    (q[:, 2] * area).sum(), tag + 'sum h |T|') < 1e-12
        assert _err(assemble(CellDiameter(mesh) / Circumradius(mesh)
                             / CellVolume(mesh) * dx),
                    (q[:, 2] / q[:, 1]).sum(), tag + 'sum h / R') < 1e-12
        # under ds: the owning cell's
        e = mesh.edges[mesh.bfacets]
        length = numpy.hypot(*(mesh.points[e[:, 0]] - mesh.points[e[:, 1]]).T)
        assert _err(assemble(CellDiameter(mesh) * ds(mesh)),
                    (q[mesh.bfacet_cell, 2] * length).sum(),
                    tag + 'sum h |e| over the boundary') < 1e-12


def _peclet_form(mesh):
    '''xi(Pe) with Pe = |b| h / (2 eps) for a P2 field b that is exactly zero
    left of the median vertex abscissa and gives Pe of about 0.1 .. 50 right
    of it.  Returns (b, Pe, xi, Pe at the points of the degree-8 rule, the
    cancellation figure).  In the cells the cut crosses the interpolant
    passes from 0 to its value beyond, so single quadrature points see a
    small positive Pe, where 1 / tanh(Pe) - 1 / Pe cancels: one ulp of tanh
    is an error of 2.2e-16 / Pe^2 in xi at that point.  Pe is proportional to
    h, the weight of a point to h^2: the cancellation figure is the sum of
    w_q |T| 2.2e-16 / Pe_q^2 over the cell, the largest over the cells --
    what one ulp of tanh can move a cell's contribution by, computed on the
    host from the inputs alone.  The test requires it a decade under its
    bound relative to the quantities compared.'''
    W = fem.VectorFunctionSpace(mesh, 'CG', 2)
    q = cref.cell_quantities(mesh)
    hmin, hmax = q[:, 2].min(), q[:, 2].max()
    eps = 0.01
    # |b| between b0 and b1 where it is not zero: Pe from 1.5 on the smallest
    # cell (the cells the cut crosses supply the values below, 0.01 .. 1) to
    # 50 on the largest
    b0, b1 = 1.5 * 2 * eps / hmin, 50 * 2 * eps / hmax
    b1 = max(b1, 2 * b0)
    xmax = float(mesh.points[:, 0].max())
    xm = float(numpy.median(mesh.points[:, 0]))

    def mag(x, y):
        s = numpy.clip((x - xm) / (xmax - xm), 0.0, 1.0)
        return numpy.where(x > xm, b0 + (b1 - b0) * s, 0.0)

    b = _field(W, [lambda x, y: 0.8 * mag(x, y), lambda x, y: 0.6 * mag(x, y)])
    Pe = sqrt(dot(b, b)) * CellDiameter(mesh) / (2 * eps)
    ctx = cref.CellContext(mesh, 8)
    with numpy.errstate(all='ignore'):
        pe = cref.evaluate(Pe.comps, ctx)
        ulp = numpy.where(pe > 1e-5, 2.2e-16 / pe**2, 0.0)
    moved = (ulp * ctx.cells.wts[None, :] * ctx.cells.adet[:, None]).sum(axis=1)
    xi = conditional(gt(Pe, 1e-5), (1 / tanh(Pe) - 1 / Pe) / Pe,
                     1.0 / 3 - Pe**2 / 45)
    return b, Pe, xi, pe, float(moved.max()), float(moved.sum())


def test_singular_untaken_branch(hip):
    '''At Pe == 0 the untaken branch is inf - inf: the result must be the
    series' 1/3 (the inputs: _peclet_form).'''
    for m, mesh in enumerate(_meshes()):
        b, Pe, xi, pe, moved, moved_sum = _peclet_form(mesh)
        print('mesh %d: Pe == 0 at %d points, smallest positive %.3g, '
              'largest %.3g' % (m, (pe == 0).sum(), pe[pe > 0].min(),
                                pe.max()))
        assert (pe == 0).sum() > 0 and pe.max() > 5.0
        # nothing in the window just above the switch
        assert not ((pe > 0) & (pe < 1e-4)).any()
        # where b vanishes on a whole cell the integrand is exactly 1/3
        assert (pe == 0).all(axis=1).sum() > 0
        form = xi * dx(mesh, degree=8)
        want = cref.functional(form)
        print('mesh %d: one ulp of tanh moves the functional by %.1e of it'
              % (m, moved_sum / abs(want)))
        assert moved_sum / abs(want) < 1e-13
        got = assemble(form)
        assert numpy.isfinite(got)
        assert _err(got, want, 'mesh %d xi(Pe) functional' % m) < 1e-12
        V = fem.FunctionSpace(mesh, 'CG', 1)
        v = TestFunction(V)
        L = xi * v * dx(degree=8)
        ref = cref.vector(L)
        # (an entry gathers about six cells)
        print('mesh %d: ... an entry of the vector by %.1e of the largest'
              % (m, 6 * moved / numpy.abs(ref).max()))
        assert 6 * moved / numpy.abs(ref).max() < 1e-13
        vec = assemble(L).get_local()
        assert numpy.isfinite(vec).all()
        assert _err(vec, ref, 'mesh %d xi(Pe) vector' % m) < 1e-12


def test_eq_and_ne_on_exact_ties(hip):
    '''The opcodes eq and ne on the device: the components of the P2 field
    of _peclet_form are EXACTLY zero on every cell left of the cut (all six
    dofs are zero there, on the device as in numpy) and not zero right of
    it.  1 / b is infinite in the untaken branch.'''
    for m, mesh in enumerate(_meshes()):
        b, Pe, xi, pe, _, _ = _peclet_form(mesh)
        X = SpatialCoordinate(mesh)
        zero = (pe == 0).all(axis=1).sum()
        assert 0 < zero < mesh.num_cells()
        c = conditional(eq(b[0], 0.0), 2.0 + X[0], tanh(b[0])) \
            + conditional(ne(b[1], 0.0), 1.0 / b[1], CellDiameter(mesh))
        form = c * dx(mesh, degree=4)
        got = assemble(form)
        assert numpy.isfinite(got)
        assert _err(got, cref.functional(form),
                    'mesh %d eq / ne functional' % m) < 1e-12
        V = fem.FunctionSpace(mesh, 'CG', 1)
        v = TestFunction(V)
        L = c * v * dx(degree=4)
        vec = assemble(L).get_local()
        assert numpy.isfinite(vec).all()
        assert _err(vec, cref.vector(L), 'mesh %d eq / ne vector' % m) < 1e-12
        # both sides of both conditions occur: counting cells with eq alone
        count = conditional(eq(b[0], 0.0), 1.0, 0.0) / CellVolume(mesh)
        n0 = assemble(count * dx(mesh, degree=0))
        n1 = assemble(conditional(ne(b[0], 0.0), 1.0, 0.0)
                      / CellVolume(mesh) * dx(mesh, degree=0))
        print('mesh %d: b == 0 at the centroid of %.1f cells, != 0 of %.1f'
              % (m, n0, n1))
        assert abs(n0 + n1 - mesh.num_cells()) < 1e-9 * mesh.num_cells()
        assert n0 > zero - 0.5 and n1 > 0.5


def test_deterministic(hip):
    mesh = _meshes()[1]
    th, w, c1, c2, c3 = _coefficients(mesh)
    V = fem.FunctionSpace(mesh, 'CG', 2)
    u, v = TrialFunction(V), TestFunction(V)
    a = (c3 * inner(grad(u), grad(v)) + c1 * u * v) * dx
    L = c2 * v * dx
    f = (c1 + c2) * dx(mesh) + c3 * ds(mesh)
    assert numpy.array_equal(_vals(assemble(a)), _vals(assemble(a)))
    assert numpy.array_equal(assemble(L).get_local(), assemble(L).get_local())
    assert assemble(f) == assemble(f)


def _conv(W):
    return _field(W, [lambda x, y: 1.0 + x * y - y**2,
                      lambda x, y: 0.5 * x**2 - y])


def _tau_conditioning(tau):
    '''What one rounding error of 2.2e-16 in tanh(Pe) or 1 / Pe moves tau by,
    relative to the largest tau: xi = (1 / tanh(Pe) - 1 / Pe) / Pe subtracts
    two numbers of size 1 / Pe, so the error of xi is 2.2e-16 / Pe^2 and that
    of tau = h^2 / (4 eps p) xi is 2.2e-16 eps p / |b|^2 -- set by the
    diffusion and the convection alone, not by the mesh.  From the inputs,
    on the host.'''
    W = tau.convection.function_space()
    B = tau.convection.array().reshape(2, W.N)[:, W.layout.cell_dofs[:, :3]]
    nb2 = B[0]**2 + B[1]**2
    return float((2.2e-16 * tau.epsilon * tau.p / nb2[nb2 > 1e-20]).max()
                 / cref.supg_tau(tau).max())


def test_tau_kernel(hip):
    '''flow_supg_tau against the tau of the heat assembly
    (cell_vertex_values): the same device function on the same inputs,
    measured bit-identical on the three meshes for p = 1, 2 -- equality is
    asserted.  Against the numpy restatement (bound 1e-12 relative to the
    largest tau) the inputs must leave the formula well conditioned
    (_tau_conditioning): with the heat case's kappa = 0.37 and |b| ~ 1 one
    rounding of tanh moves tau by 4e-14 .. 1.2e-11 of its maximum (measured
    differences: 3.9e-14, 2.0e-13, 5.2e-12 on meshes 0, 0, 1 -- the
    prediction), a property of the formula in fp64 that both sides share.
    The numpy comparison therefore runs at kappa = 0.0037 (Pe 0.4 .. 15,
    both branches of xi's switch are far), where that figure is required
    below 1e-14.'''
    for m, mesh in enumerate(_meshes()):
        W = fem.VectorFunctionSpace(mesh, 'CG', 2)
        conv = _conv(W)
        nc = mesh.num_cells()
        for p in (1, 2):
            tau = stabilization.supg(mesh, conv, 0.37, p)
            old = tau.cell_vertex_values()                          # (Nc, 3)
            new = tau.form_lattice(mesh).values.cpu().numpy().reshape(3, nc).T
            _err(new, old, 'mesh %d p = %d tau: kernel vs assembly' % (m, p))
            assert numpy.array_equal(new, old)
            tau = stabilization.supg(mesh, conv, 0.0037, p)
            figure = _tau_conditioning(tau)
            print('mesh %d p = %d: one rounding of tanh moves tau by %.1e'
                  % (m, p, figure))
            assert figure < 1e-14
            new = tau.form_lattice(mesh).values.cpu().numpy().reshape(3, nc).T
            assert numpy.array_equal(new, tau.cell_vertex_values())
            assert _err(new, cref.supg_tau(tau),
                        'mesh %d p = %d tau: kernel vs numpy' % (m, p)) < 1e-12
    # a convection field that is zero somewhere: tau = 0 there
    mesh = _meshes()[0]
    W = fem.VectorFunctionSpace(mesh, 'CG', 2)
    conv = _field(W, [lambda x, y: numpy.where(x > 0.5, 1.0, 0.0),
                      lambda x, y: 0.0 * x])
    tau = stabilization.supg(mesh, conv, 0.1, 1)
    lat = tau.form_lattice().values.cpu().numpy().reshape(3, -1).T
    xv = mesh.points[mesh.cell_vertices][:, :, 0]
    assert (lat[xv <= 0.5] == 0.0).all() and (lat[xv > 0.5] > 0.0).all()
    # tau > 1e3 raises, on this path as in the assembly
    # (for Pe -> infinity tau -> h / (2 |b|), whatever the diffusion: a slow
    # field, |b| = 1e-6, at Pe of about 50)
    slow = _field(W, [lambda x, y: 1.0e-6 + 0.0 * x, lambda x, y: 0.0 * x])
    fast = stabilization.supg(mesh, slow, 1.0e-9, 1)
    with pytest.raises(RuntimeError, match='tau > 1e3'):
        fast.cell_vertex_values()
    with pytest.raises(RuntimeError, match='tau > 1e3'):
        fast.form_lattice()
    V = fem.FunctionSpace(mesh, 'CG', 1)
    v = TestFunction(V)
    with pytest.raises(RuntimeError, match='tau > 1e3'):
        assemble(fast * v * dx)
    # after conv.set_array the next assemble uses the new tau
    conv = _conv(W)
    tau = stabilization.supg(mesh, conv, 0.37, 1)
    L = tau * dot(conv, grad(v)) * dx
    first = assemble(L).get_local()
    assert _err(first, cref.vector(L), 'tau form, first field') < 1e-12
    conv.set_array(2.5 * conv.array()[::-1].copy())
    second = assemble(L).get_local()
    assert _err(second, cref.vector(L), 'tau form, after set_array') < 1e-12
    assert numpy.abs(second - first).max() > 1e-3 * numpy.abs(first).max()
    # a functional of tau alone, and tau under ds
    f = tau * dx(mesh) + tau * ds(mesh)
    assert _err(assemble(f), cref.functional(f), 'tau dx + ds') < 1e-12


def _supg_forms(V, conv, kappa, rho, cp, source):
    '''M's forms and f as reference flow/heat.py writes them, minus the
    div(kappa grad(u)) term of R2 (zero on P1).'''
    u, v = TrialFunction(V), TestFunction(V)
    mesh = V.mesh()
    rho_cp = rho * cp
    kap = fem.Constant(kappa)
    tau = stabilization.supg(mesh, conv, kappa, V.degree)
    mass = u * v * dx
    msupg = u * tau * dot(conv, grad(v)) * dx
    f = - kap * dot(grad(u), grad(v / rho_cp)) * dx \
        - dot(conv, grad(u)) * v * dx \
        + source * v * dx
    R2 = - dot(conv, grad(u)) + source / rho_cp
    f += R2 * tau * dot(conv, grad(v)) * dx
    return mass, msupg, f, tau


def test_supg_heat_operator_from_form_text(hip):
    '''P1: M, A and b of Heat(..., supg_stabilization=True) entry by entry.
    The estimated degrees (u tau conv.grad v: 4; conv.grad u tau conv.grad v
    and source tau conv.grad v: 5) lie within the dedicated kernel's fixed
    16-point rule (exact for degree 7): both sides integrate exactly, no
    metadata is needed.'''
    fcp = {'quadrature_rule': 'vertex', 'representation': 'quadrature'}
    for m, mesh in enumerate(_meshes()):
        W = fem.VectorFunctionSpace(mesh, 'CG', 2)
        conv = _conv(W)
        source = fem.Expression('1.0 + x[0]*x[1] - 2.0*x[1]*x[1]', degree=2)
        kappa, rho, cp = 0.37, 1.3, 2.1
        V = fem.FunctionSpace(mesh, 'CG', 1)
        heat = Heat(V, conv, kappa, rho, cp, [], source,
                    supg_stabilization=True)
        mass, msupg, f, _ = _supg_forms(V, conv, kappa, rho, cp, source)
        M = _vals(assemble(mass, form_compiler_parameters=fcp)) \
            + _vals(assemble(msupg))
        A, b = assemble_system(lhs(f), rhs(f))
        tag = 'mesh %d P1 SUPG heat ' % m
        assert _err(M, _vals(heat.M), tag + 'M') < 1e-12
        assert _err(_vals(A), _vals(heat.A), tag + 'A') < 1e-12
        assert _err(b.get_local(), heat.b.get_local(), tag + 'b') < 1e-12


def test_supg_heat_operator_p2_against_evaluator(hip):
    '''P2: the M part and the first-order parts against the evaluator only
    (the second-order term of R2 stays refused); tau's vertex values are
    data for the evaluator.'''
    fcp = {'quadrature_rule': 'vertex', 'representation': 'quadrature'}
    for m, mesh in enumerate(_meshes()):
        W = fem.VectorFunctionSpace(mesh, 'CG', 2)
        conv = _conv(W)
        source = fem.Expression('1.0 + x[0]*x[1] - 2.0*x[1]*x[1]', degree=2)
        V = fem.FunctionSpace(mesh, 'CG', 2)
        mass, msupg, f, tau = _supg_forms(V, conv, 0.37, 1.3, 2.1, source)
        # (at kappa = 0.37 the formula of tau is conditioned to 1e-11 only,
        # test_tau_kernel: the evaluator interpolates the vertex values of
        # the heat assembly's tau, which that test ties to flow_supg_tau bit
        # for bit and to numpy where the formula allows it)
        cref.give_lattice(tau, tau.cell_vertex_values())
        tag = 'mesh %d P2 SUPG heat ' % m
        assert _err(assemble(msupg).to_scipy(), cref.matrix(msupg),
                    tag + 'M supg') < 1e-12
        assert _err(assemble(mass, form_compiler_parameters=fcp).to_scipy(),
                    cref.matrix(mass, fcp), tag + 'M lumped') < 1e-12
        assert _err(assemble(lhs(f)).to_scipy(), cref.matrix(lhs(f)),
                    tag + 'A') < 1e-12
        assert _err(assemble(rhs(f)).get_local(), cref.vector(rhs(f)),
                    tag + 'b') < 1e-12


def _clipped_problem(n, degree):
    '''-div(k_eff grad u) + b . grad u = f on the unit square, k(u) = k0 (1 +
    u^2), k_eff = k + max_value(0, c h |b| - k) (artificial viscosity where
    the cell Peclet number is large: c h |b| = 0.069 against k between 0.05
    and 0.1, so both sides of the clip occur and the problem is nonlinear), f manufactured for the unclipped operator from
    u_exact = sin(pi x) sin(pi y); Dirichlet data.'''
    mesh = fem.UnitSquareMesh(n, n)
    V = fem.FunctionSpace(mesh, 'CG', degree)
    W = fem.VectorFunctionSpace(mesh, 'CG', 2)
    b = _field(W, [lambda x, y: 1.0 + 0.0 * x, lambda x, y: 0.5 + 0.0 * x])
    k0, c = 0.05, 0.35
    S = 'sin(pi*x[0])*sin(pi*x[1])'
    G = ('pi*pi*(pow(cos(pi*x[0])*sin(pi*x[1]), 2)'
         ' + pow(sin(pi*x[0])*cos(pi*x[1]), 2))')
    conv = 'pi*cos(pi*x[0])*sin(pi*x[1]) + 0.5*pi*sin(pi*x[0])*cos(pi*x[1])'
    f = fem.Expression(('%g*(2.0*pi*pi*S*(1.0 + S*S) - 2.0*S*G) + C' % k0)
                       .replace('S', '(%s)' % S).replace('G', '(%s)' % G)
                       .replace('C', '(%s)' % conv), degree=5)
    u = fem.Function(V)
    v = TestFunction(V)
    k = k0 * (1 + u**2)
    k_eff = k + max_value(0.0, c * CellDiameter(mesh) * sqrt(dot(b, b)) - k)
    F = k_eff * inner(grad(u), grad(v)) * dx + dot(b, grad(u)) * v * dx \
        - f * v * dx
    bcs = [fem.DirichletBC(V, fem.Expression(S, degree=5), 'on_boundary')]
    return V, u, F, bcs


def test_newton_with_a_clipped_coefficient(hip):
    '''solve(F == 0) against the host Newton of conditional_reference (the
    evaluator's J and F, sparse LU): the same iteration count and the
    solution to 1e-7 relative l2, the bound of the other nonlinear solves.'''
    for degree in (1, 2):
        V, u, F, bcs = _clipped_problem(8, degree)
        info = fem.solve(F == 0, u, bcs)
        assert info.converged
        Vr, ur, Fr, bcr = _clipped_problem(8, degree)
        res, its = cref.host_newton(Fr, ur, bcr)
        print('P%d residuals, device: %s' % (degree, info.residuals))
        print('P%d residuals, host:   %s' % (degree, res))
        assert info.iterations == its
        e = numpy.linalg.norm(u.array() - ur.array()) \
            / numpy.linalg.norm(ur.array())
        print('P%d: %r; rel l2 vs host Newton %.2e' % (degree, info, e))
        assert e < 1e-7
