# -*- coding: utf-8 -*-
'''
flow_mass_correct (the velocity correction's increment solve around the
caller's vectors) against the route it replaces, BIT FOR BIT.  The reference
is the old route, which stays in the library:

    start = copy(ui); flow_bc_set_values(start); flow_bc_set_values(0 -> d0);
    flow_mass_solve_increment(g, start, d0) -> u1; inc = copy(u1); inc -= ui

u1, the filed increment, the count of corrections and the reported |z| must be
equal under numpy.array_equal, however the solve ends.

Rows per component / nonzeros / fp16 tiles (<= 2044 nonzeros, <= 256 rows) /
fp64 tiles, none a multiple of 256 or of a tile:
    UnitSquareMesh(5, 4, 'crossed')        P1   50 /  308 / 1 / 1
                                           P2  179 / 1913 / 1 / 2
    karman_channel(24, 7, fitted=True)     P1  199 / 1253 / 1 / 2
                                           P2  726 / 7824 / 4 / 8
    KarmanProblem(48, 11) (whole steps)    P2 2222 / 24608 / 13 / 25
(karman_channel(24, 6, fitted=True) does not exist: with ny = 6 the blend zone
of the fitted hole, three block half-sides either way, touches the channel
wall and the mesh generator refuses; ny = 7 is the nearest that it builds.)
'''
import numpy
import pytest
import torch

from flow_amd import fem, _hip, device, karman
from flow_amd.fem import mass as fmass
from flow_amd.fem import ops
from flow_amd.navier_stokes import pressure_correction as pc

EPS = 1.0e-12


class _Left(fem.SubDomain):
    def inside(self, x, on_boundary):
        return on_boundary & (x[0] < EPS)


class _Bottom(fem.SubDomain):
    def inside(self, x, on_boundary):
        return on_boundary & (x[1] < EPS)


def _mesh(name):
    if name == 'square':
        return fem.UnitSquareMesh(5, 4, 'crossed')
    return fem.karman_channel(24, 7, fitted=True)


def _conditions(name, W, which):
    '''Dirichlet sets with a component-only ("inflow"-style) condition, so that
    the two planes of the mask differ.'''
    if name == 'square':
        prof = fem.Expression('1.0 + x[1] * (1.0 - x[1])', degree=2)
        if which == 'component-only':
            return [fem.DirichletBC(W.sub(0), prof, _Left())]
        return [fem.DirichletBC(W, (0.25, -0.5), _Bottom()),
                fem.DirichletBC(W.sub(0), prof, _Left())]
    prof = fem.Expression('0.01 * (0.07 - x[1]) * (x[1] + 0.07) / 0.0049',
                          degree=2)
    if which == 'component-only':
        return [fem.DirichletBC(W.sub(0), prof, karman.LeftBoundary()),
                fem.DirichletBC(W.sub(0), prof, karman.RightBoundary())]
    return [fem.DirichletBC(W, (0.0, 0.0), karman.UpperBoundary()),
            fem.DirichletBC(W, (0.0, 0.0), karman.LowerBoundary()),
            fem.DirichletBC(W, (0.0, 0.0), karman.ObstacleBoundary()),
            fem.DirichletBC(W.sub(0), prof, karman.LeftBoundary()),
            fem.DirichletBC(W.sub(0), prof, karman.RightBoundary())]


class _Setup(object):
    '''Everything both routes share for one (mesh, degree, condition set),
    built once.'''
    def __init__(self, name, deg, which):
        mesh = _mesh(name)
        W = fem.VectorFunctionSpace(mesh, 'Lagrange', deg)
        lay = W.layout
        self.n, self.n2 = W.N, W.size()
        M = ops.assemble_mass(W)
        dofs, self.bc_dofs, self.bc_vals = pc._bc_arrays(
            _conditions(name, W, which), self.n2)
        self.nbc = self.bc_dofs.numel()
        assert self.nbc > 0
        free = numpy.ones(self.n2, dtype=numpy.uint8)
        free[dofs] = 0
        # the two planes' masks differ
        assert not numpy.array_equal(free[:self.n], free[self.n:])
        self.free = free
        self.A = ops.Matrix(lay, 4, M.vals, rowmask=device.to_device(free))
        self.dinv = self.A.diag_inv()
        self.solver = fmass.MassSolver(self.A, self.dinv)
        self.xbc = pc._bc_full(lay, dofs, self.bc_dofs, self.bc_vals, self.n2)
        self.zeros = _hip.fill(device.empty(self.nbc), 0.0)
        rng = numpy.random.RandomState(11 + deg)
        xy = lay.dof_coords
        smooth = numpy.concatenate([numpy.sin(3.0 * xy[:, 0]) + xy[:, 1],
                                    numpy.cos(2.0 * xy[:, 1]) - xy[:, 0]])
        self.ui = device.to_device(smooth + 0.1 * rng.standard_normal(self.n2))
        g = 1.0e-4 * rng.standard_normal(self.n2)
        self.g = device.to_device(g)
        _hip.check(_hip.lib().flow_bc_set_values(
            self.nbc, _hip.i32(self.bc_dofs), _hip.f64(self.zeros),
            _hip.f64(self.g), _hip.stream()))
        # start vectors of the increment: non-zero ON the Dirichlet rows
        self.d_near = 1.0e-3 * (smooth + 1.5)
        self.d_far = 1.0e3 * (smooth + 1.5)
        assert (self.d_near[free == 0] != 0.0).all()


_SETUPS = {}


def _setup(name, deg, which):
    key = (name, deg, which)
    if key not in _SETUPS:
        _SETUPS[key] = _Setup(*key)
    return _SETUPS[key]


def _nan(n):
    return torch.full((n,), float('nan'), dtype=torch.float64,
                      device=device.get())


def _old_route(s, solver, d0, tol, maxit):
    lib = _hip.lib()
    st = _hip.stream()
    start = _hip.clone(s.ui)
    _hip.check(lib.flow_bc_set_values(
        s.nbc, _hip.i32(s.bc_dofs), _hip.f64(s.bc_vals), _hip.f64(start), st))
    dd = None
    if d0 is not None:
        dd = device.to_device(d0)
        _hip.check(lib.flow_bc_set_values(
            s.nbc, _hip.i32(s.bc_dofs), _hip.f64(s.zeros), _hip.f64(dd), st))
    u1 = _nan(s.n2)
    sol = err = None
    try:
        sol = solver.solve_increment(s.g, start, u1, tol, maxit=maxit,
                                     delta0=dd)
    except _hip.NotConverged as e:
        err = str(e)
    inc = _nan(s.n2)
    ops.copy(inc, u1)
    ops.axpby(-1.0, s.ui, 1.0, inc)
    return u1.cpu().numpy(), inc.cpu().numpy(), sol, err


def _new_route(s, solver, d0, tol, maxit):
    dd = device.to_device(d0) if d0 is not None else None
    u1, inc = _nan(s.n2), _nan(s.n2)
    ui_before = s.ui.cpu().numpy()
    sol = err = None
    try:
        sol = solver.correct(s.g, s.ui, s.xbc, s.bc_dofs, u1, tol, maxit=maxit,
                             delta0=dd, inc_out=inc)
    except _hip.NotConverged as e:
        err = str(e)
    assert numpy.array_equal(s.ui.cpu().numpy(), ui_before)
    return u1.cpu().numpy(), inc.cpu().numpy(), sol, err


def _same(old, new):
    u_old, i_old, sol_old, err_old = old
    u_new, i_new, sol_new, err_new = new
    assert numpy.isfinite(u_old).all() and numpy.isfinite(i_old).all()
    assert numpy.array_equal(u_new, u_old)
    assert numpy.array_equal(i_new, i_old)
    assert err_new == err_old
    if sol_old is not None:
        assert sol_new.iterations == sol_old.iterations
        assert sol_new.residual == sol_old.residual
        assert sol_new.method == sol_old.method


CASES = [(name, deg, which)
         for name in ('square', 'karman')
         for deg in (2, 1)
         for which in ('walls+component', 'component-only')]


@pytest.mark.gpu
@pytest.mark.parametrize('name,deg,which', CASES)
def test_new_entry_is_the_old_route_bit_for_bit(hip, name, deg, which):
    '''Both start cases -- none (the first defect is D^-1 g, no product) and a
    start vector that is non-zero on the Dirichlet rows before masking --, a
    far start that needs several corrections (the first reads the caller's
    vector, the later ones the solver's), and the unconverged exit.'''
    s = _setup(name, deg, which)
    tol = 1.0e-10
    # no start vector
    old = _old_route(s, s.solver, None, tol, 50)
    new = _new_route(s, s.solver, None, tol, 50)
    _same(old, new)
    assert old[3] is None and old[2].iterations >= 1
    # the boundary values are in u1 on the Dirichlet rows, not ui's
    bcv = s.xbc.cpu().numpy()
    assert numpy.array_equal(new[0][s.free == 0], bcv[s.free == 0])
    # a near start vector
    old = _old_route(s, s.solver, s.d_near, tol, 50)
    new = _new_route(s, s.solver, s.d_near, tol, 50)
    _same(old, new)
    assert old[3] is None
    assert numpy.array_equal(new[0][s.free == 0], bcv[s.free == 0])
    # a far one: at least two corrections
    old = _old_route(s, s.solver, s.d_far, tol, 50)
    new = _new_route(s, s.solver, s.d_far, tol, 50)
    _same(old, new)
    assert old[3] is None and old[2].iterations >= 2, old[2]
    # more corrections enqueued than needed before the first look: the same
    # (everything behind the deciding correction is a no-op)
    for d0 in (None, s.d_far):
        dd = device.to_device(d0) if d0 is not None else None
        u1, inc = _nan(s.n2), _nan(s.n2)
        sol = s.solver.correct(s.g, s.ui, s.xbc, s.bc_dofs, u1, tol, maxit=50,
                               delta0=dd, inc_out=inc, first_check=9)
        ref = _old_route(s, s.solver, d0, tol, 50)
        _same(ref, (u1.cpu().numpy(), inc.cpu().numpy(), sol, None))


@pytest.mark.gpu
@pytest.mark.parametrize('name,deg,which', CASES)
def test_unconverged_exit_leaves_the_same_vectors(hip, name, deg, which):
    '''maxit = 1 with a tolerance one correction cannot meet: the same error,
    the same u1, the same increment -- with and without a start vector.'''
    s = _setup(name, deg, which)
    for d0 in (None, s.d_far):
        old = _old_route(s, s.solver, d0, 1.0e-15, 1)
        new = _new_route(s, s.solver, d0, 1.0e-15, 1)
        assert old[3] is not None and 'did not converge in 1' in old[3], old
        _same(old, new)
    # two corrections, still not enough: the second one wrote last
    old = _old_route(s, s.solver, s.d_far, 1.0e-15, 2)
    new = _new_route(s, s.solver, s.d_far, 1.0e-15, 2)
    assert old[3] is not None
    _same(old, new)


@pytest.mark.gpu
def test_without_an_increment_vector_and_plain_stream(hip):
    '''inc_out is optional, and the plain fp16 stream (no packed words) runs
    the same last step.'''
    s = _setup('karman', 2, 'walls+component')
    plain = fmass.MassSolver(s.A, s.dinv, packed=False)
    assert plain.packed16 is None and s.solver.packed16 is not None
    for d0 in (None, s.d_far):
        old = _old_route(s, plain, d0, 1.0e-10, 50)
        new = _new_route(s, plain, d0, 1.0e-10, 50)
        _same(old, new)
        packed = _new_route(s, s.solver, d0, 1.0e-10, 50)
        _same(old, packed)
        u1 = _nan(s.n2)
        dd = device.to_device(d0) if d0 is not None else None
        s.solver.correct(s.g, s.ui, s.xbc, s.bc_dofs, u1, 1.0e-10, delta0=dd)
        assert numpy.array_equal(u1.cpu().numpy(), old[0])


@pytest.mark.gpu
def test_fallback_gives_what_the_old_route_gives(hip):
    '''A Chebyshev interval that misses the spectrum: the watch on the
    contraction gives the iteration up (kDone == 3), both routes fall back to
    Jacobi-CG, and u1 and the increment are the same.'''
    s = _setup('karman', 2, 'walls+component')
    bad = fmass.MassSolver(s.A, s.dinv)
    bad.struct.lam_max = 0.3 * s.solver.struct.lam_max
    bad.struct.lam_min = 0.3 * s.solver.struct.lam_min
    old = _old_route(s, bad, s.d_near, 1.0e-10, 50)
    assert bad.fallbacks == 1 and 'cg' in old[2].method
    new = _new_route(s, bad, s.d_near, 1.0e-10, 50)
    assert bad.fallbacks == 2
    _same(old, new)


@pytest.mark.gpu
def test_whole_steps_are_the_same_on_both_routes(hip):
    '''KarmanProblem(48, 11): three steps under the step-size controller, then
    two at a fixed step (the start vectors of the increment only count while
    the step size is settled), with the new route and with the old one:
    velocity, pressure and dt bit for bit after each step.'''
    par = pc.solver_parameters['correction']
    assert par['around_caller'] is True            # the default
    runs = {}
    try:
        for around in (True, False):
            par['around_caller'] = around
            prob = karman.KarmanProblem(48, 11)
            prob.set_initial_profile()
            prob.dt = 2.0e-3
            states = []
            for k in range(5):
                prob.step(adapt=k < 3)
                states.append((prob.u0.data.cpu().numpy().copy(),
                               prob.p0.data.cpu().numpy().copy(), prob.dt))
            runs[around] = states
            # (the increments were filed: the later steps had a history)
            hist = pc.start_vectors._state(prob.W.layout).trajectories
            assert max(len(t.hist.get('correction_increments', []))
                       for t in hist) >= 3
    finally:
        par['around_caller'] = True
    for k, (new, old) in enumerate(zip(runs[True], runs[False])):
        assert numpy.isfinite(new[0]).all() and numpy.isfinite(new[1]).all()
        assert new[2] == old[2], (k, new[2], old[2])
        assert numpy.array_equal(new[0], old[0]), k
        assert numpy.array_equal(new[1], old[1]), k
