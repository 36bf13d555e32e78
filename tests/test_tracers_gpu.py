# -*- coding: utf-8 -*-
'''
Tracer particles on the HIP path (flow_amd/fem/tracers.py; csrc/
form_kernels.hip: advect_points_kernel): closed forms (rigid rotation, a
velocity linear in time, the exit through the outflow), the numpy restatement
of tests/tracer_reference.py on fields that are not linear, the state a call
leaves behind against a fresh Probes, determinism, and the bookkeeping.

Bounds.  Closed forms: max(10 e_ref, 1e-12) of the domain diameter, e_ref
the deviation of the restatement itself from the closed form for the same
case (computed here from the restatement, never from the device's result).
Restatement: tol = 64 eps * 4 steps * A * D -- 64 ulp per stage evaluation,
carried by the amplification A the restatement shows when its starts are
moved by 1e-10 D (tracer_reference.nonlinear_reference); particles one of
whose stage points comes within 1e-6 D of the boundary are left out (rounding
may decide whether they are lost), at most 5 % per case.

Every test prints its measured error next to its bound (pytest -s).
'''
import numpy
import pytest

from flow_amd import device, fem
from flow_amd.fem import Probes, Tracers, SpatialCoordinate, sqrt, dot

import point_reference as pref
import tracer_reference as tref

pytestmark = pytest.mark.gpu


def _state_is_consistent(tr, u):
    '''cells and values of a fresh Probes at the stored positions, bit for
    bit; NaN for the lost.'''
    pos, cells, alive = tr.positions(), tr.cells(), tr.alive()
    assert cells.dtype == numpy.int32 and alive.dtype == bool
    assert numpy.array_equal(alive, cells >= 0)
    probes = Probes(tr.mesh, pos)
    assert numpy.array_equal(cells[alive], probes.cells[alive])
    got, want = tr(u), probes(u)
    assert got.shape == (len(tr), 2)
    assert numpy.array_equal(got[alive], want[alive])
    assert numpy.isnan(got[~alive]).all()
    s = tr(sqrt(dot(u, u)))
    assert s.shape == (len(tr),) and numpy.isnan(s[~alive]).all()
    assert numpy.array_equal(s[alive], probes(sqrt(dot(u, u)))[alive])
    # the stored barycentrics put the particle where it is
    x = tr(SpatialCoordinate(tr.mesh))
    assert numpy.abs(x[alive] - pos[alive]).max() \
        <= 1e-14 * numpy.abs(tr.mesh.points).max()


@pytest.mark.parametrize('sign', [1, -1])
@pytest.mark.parametrize('deg', [1, 2])
@pytest.mark.parametrize('scheme', tref.SCHEMES)
@pytest.mark.parametrize('kind', ['square', 'channel'])
def test_rigid_rotation(hip, kind, scheme, deg, sign):
    mesh, c, starts = tref.rotation_case(kind)
    u = tref.rotation_field(mesh, deg, c)
    dt, steps = sign * tref.ROTATION_DT, tref.ROTATION_STEPS
    want = tref.rotation_closed_form(c, starts, scheme, dt, steps)
    D = tref.diameter(mesh)
    ref_pos, ref_cells, _ = tref.advect(mesh, starts, u, dt, steps, scheme,
                                        distances=False)
    e_ref = numpy.abs(ref_pos - want).max() / D
    tr = Tracers(mesh, starts)
    assert len(tr) == len(starts) and tr.alive().all()
    assert tr.advect(u, dt, steps=steps, scheme=scheme) is None
    err = numpy.abs(tr.positions() - want).max() / D
    bound = max(10.0 * e_ref, 1e-12)
    print('rotation %-7s %-5s P%d dt %+.2f: error %.2e  e_ref %.2e  bound %.2e'
          % (kind, scheme, deg, dt, err, e_ref, bound))
    assert tr.alive().all()
    assert err <= bound
    _state_is_consistent(tr, u)


@pytest.mark.parametrize('deg', [1, 2])
def test_time_interpolation(hip, deg):
    mesh = fem.UnitSquareMesh(12, 9)
    u0 = tref.constant_field(mesh, deg, 1.0)
    u1 = tref.constant_field(mesh, deg, 3.0)
    starts = numpy.array([[0.1, 0.3], [0.2, 0.77], [0.05, 0.5]])
    dt, steps = 0.02, 10
    D = tref.diameter(mesh)
    for scheme in tref.SCHEMES:
        dx = 2.0 * steps * dt if scheme != 'euler' \
            else steps * dt * (1.0 + (steps - 1.0) / steps)
        for sgn, x0 in ((1.0, starts), (-1.0, starts + [0.5, 0.0])):
            want = x0 + [sgn * dx, 0.0]
            ref_pos, _, _ = tref.advect(mesh, x0, u0, sgn * dt, steps, scheme,
                                        u_next=u1, distances=False)
            e_ref = numpy.abs(ref_pos - want).max() / D
            tr = Tracers(mesh, x0)
            tr.advect(u0, sgn * dt, steps=steps, scheme=scheme, u_next=u1)
            err = numpy.abs(tr.positions() - want).max() / D
            print('time interpolation %-5s P%d dt %+.2f: error %.2e  e_ref %.2e'
                  % (scheme, deg, sgn * dt, err, e_ref))
            assert tr.alive().all()
            assert err <= max(10.0 * e_ref, 1e-12)


@pytest.mark.parametrize('deg', [1, 2])
def test_exit_exactly(hip, deg):
    '''Flags and cells equal the prediction exactly.  A lost particle keeps
    the position of the start of the substep that lost it: the bits of a run
    that stops there (a lane's path depends on its own position only), and
    the closed form start + done * dt within the bound of the closed forms
    (the basis sums to 1 to rounding only: no formula gives the bits).'''
    mesh = fem.UnitSquareMesh(12, 9)
    u = tref.constant_field(mesh, deg, 1.0)
    D = tref.diameter(mesh)
    for steps in (1, 7, 8, 10, 13, 20):
        done, lost, want = tref.exit_prediction(steps)
        ref_pos, ref_cells, dist = tref.advect(mesh, tref.EXIT_STARTS, u,
                                               tref.EXIT_DT, steps, 'rk4')
        assert dist.min() > 1e-3 and numpy.array_equal(ref_cells < 0, lost)
        e_ref = numpy.abs(ref_pos - want).max() / D
        tr = Tracers(mesh, tref.EXIT_STARTS)
        tr.advect(u, tref.EXIT_DT, steps=steps)
        pos, cells = tr.positions(), tr.cells()
        assert numpy.array_equal(cells < 0, lost)
        assert numpy.array_equal(tr.alive(), ~lost)
        assert numpy.array_equal(cells[~lost], pref.locate(mesh, pos[~lost]))
        assert numpy.array_equal(cells[lost], numpy.full(lost.sum(), -1))
        assert numpy.abs(pos - want).max() / D <= max(10.0 * e_ref, 1e-12)
        for k in numpy.unique(done[lost]):
            stop = Tracers(mesh, tref.EXIT_STARTS)
            stop.advect(u, tref.EXIT_DT, steps=int(k))
            sel = lost & (done == k)
            assert stop.alive()[sel].all()
            assert numpy.array_equal(stop.positions()[sel], pos[sel])
        # a later call leaves the lost alone
        tr.advect(u, -tref.EXIT_DT, steps=2)
        assert numpy.array_equal(tr.positions()[lost], pos[lost])
        assert numpy.array_equal(tr.cells() < 0, lost)
    assert lost.all()


@pytest.mark.parametrize('moving', [False, True])
@pytest.mark.parametrize('deg', [1, 2])
@pytest.mark.parametrize('k', range(3))
def test_against_restatement(hip, k, deg, moving):
    mesh = tref.nonlinear_meshes()[k]
    u, u_next, dt, starts = tref.nonlinear_case(mesh, k, deg)
    if not moving:
        u_next = None
    D = tref.diameter(mesh)
    ref_pos, ref_cells, out, A, tol = tref.nonlinear_reference(
        mesh, u, u_next, dt, starts)
    # the cap is a condition of the case, not a measurement
    assert out.mean() <= 0.05
    start_cells = tref.locate(mesh, starts)
    assert (start_cells < 0).sum() > 100 and (ref_cells >= 0).sum() > 1000
    assert ((ref_cells < 0) & (start_cells >= 0)).sum() > 20

    tr = Tracers(mesh, starts)
    assert numpy.array_equal(tr.cells(), start_cells)
    tr.advect(u, dt, steps=tref.NONLINEAR_STEPS, scheme='rk4', u_next=u_next)
    pos, cells = tr.positions(), tr.cells()
    keep = ~out
    err = numpy.abs(pos[keep] - ref_pos[keep]).max()
    print('restatement mesh %d P%d %s: left out %d of %d, lost %d, A %.2f, '
          'error %.2e D, tol %.2e D'
          % (k, deg, 'u_next' if moving else 'frozen', out.sum(), len(out),
             (cells < 0).sum(), A, err / D, tol / D))
    assert numpy.array_equal(cells[keep] < 0, ref_cells[keep] < 0)
    assert err <= tol
    live = keep & (cells >= 0)
    assert numpy.array_equal(cells[live], ref_cells[live])
    # particles that start outside the mesh never move
    never = start_cells < 0
    assert numpy.array_equal(pos[never], starts[never])
    assert (cells[never] < 0).all()
    _state_is_consistent(tr, u)


def test_determinism(hip):
    mesh = tref.nonlinear_meshes()[1]
    u, u_next, dt, starts = tref.nonlinear_case(mesh, 1, 2)

    def run(pts, calls, steps, nxt):
        tr = Tracers(mesh, pts)
        for _ in range(calls):
            tr.advect(u, dt, steps=steps, u_next=nxt)
        return tr.positions(), tr.cells(), tr.alive()

    for nxt in (None, u_next):
        a = run(starts, 1, 20, nxt)
        b = run(starts, 1, 20, nxt)
        perm = numpy.random.RandomState(7).permutation(len(starts))
        c = run(starts[perm], 1, 20, nxt)
        for x, y, z in zip(a, b, c):
            assert numpy.array_equal(x, y)
            assert numpy.array_equal(x[perm], z)
        assert (~a[2]).sum() > 300 and a[2].sum() > 1000
    # twenty calls of one substep are one call of twenty on a frozen field
    a = run(starts, 1, 20, None)
    b = run(starts, 20, 1, None)
    for scheme in ('euler', 'rk2'):
        t1, t2 = Tracers(mesh, starts), Tracers(mesh, starts)
        t1.advect(u, -dt, steps=6, scheme=scheme)
        for _ in range(6):
            t2.advect(u, -dt, steps=1, scheme=scheme)
        assert numpy.array_equal(t1.positions(), t2.positions())
        assert numpy.array_equal(t1.cells(), t2.cells())
    for x, y in zip(a, b):
        assert numpy.array_equal(x, y)


def test_inject_and_compact(hip):
    mesh = tref.nonlinear_meshes()[2]
    u, _, dt, starts = tref.nonlinear_case(mesh, 2, 2)
    tr = Tracers(mesh, starts[:500])
    tr.advect(u, dt, steps=10)
    pos, cells = tr.positions(), tr.cells()
    tr.inject(starts[500:800])
    tr.inject(numpy.zeros((0, 2)))
    assert len(tr) == 800
    assert numpy.array_equal(tr.positions()[:500], pos)
    assert numpy.array_equal(tr.cells()[:500], cells)
    assert numpy.array_equal(tr.positions()[500:], starts[500:800])
    assert numpy.array_equal(tr.cells()[500:], pref.locate(mesh, starts[500:800]))
    _state_is_consistent(tr, u)
    tr.advect(u, dt, steps=10)
    pos, cells, alive = tr.positions(), tr.cells(), tr.alive()
    assert 50 < (~alive).sum() < 750
    kept = tr.compact()
    assert numpy.array_equal(kept, numpy.nonzero(alive)[0])
    assert len(tr) == alive.sum() and tr.alive().all()
    assert numpy.array_equal(tr.positions(), pos[alive])
    assert numpy.array_equal(tr.cells(), cells[alive])
    _state_is_consistent(tr, u)
    # ... and moves on as the same particles would have
    other = Tracers(mesh, pos[alive])
    tr.advect(u, dt, steps=3)
    other.advect(u, dt, steps=3)
    assert numpy.array_equal(tr.positions(), other.positions())
    _state_is_consistent(tr, u)
    # a streakline: seeds every step, the lost dropped now and then
    line = Tracers(mesh, numpy.zeros((0, 2)))
    for step in range(5):
        line.inject([(0.02, 0.0), (0.02, 0.03)])
        line.advect(u, dt, steps=4)
    assert len(line) == 10 and line.alive().sum() >= 2
    x = line.positions()[:, 0]
    assert (x[0::2][:-1] >= x[0::2][1:]).all()      # older seeds are further


def test_c_abi_refusals(hip):
    '''flow_advect_points validates its arguments itself.'''
    import ctypes
    from flow_amd import _hip
    from flow_amd.fem.ops import mesh_struct, space_struct
    from flow_amd.fem.points import _grid_struct
    mesh = fem.UnitSquareMesh(4, 4)
    W = fem.VectorFunctionSpace(mesh, 'CG', 2)
    u = fem.Function(W)
    tr = Tracers(mesh, [(0.5, 0.5)])
    lib = _hip.lib()

    def call(n=1, dt=0.1, steps=1, scheme=4, xy=tr._xy, field=u.data):
        return lib.flow_advect_points(
            ctypes.byref(mesh_struct(mesh)), ctypes.byref(_grid_struct(mesh)),
            ctypes.byref(space_struct(W.layout)),
            None if field is None else _hip.f64(field), None, n,
            None if xy is None else _hip.f64(xy), _hip.i32(tr._cell),
            _hip.f64(tr._bary), dt, steps, scheme, _hip.stream())

    assert call() == 0
    assert call(n=0, xy=None) == 0
    for bad in (dict(n=-1), dict(dt=float('nan')), dict(steps=0),
                dict(scheme=3), dict(xy=None), dict(field=None)):
        assert call(**bad) != 0
    device.synchronize()
    assert numpy.array_equal(tr.positions(), [[0.5, 0.5]])
