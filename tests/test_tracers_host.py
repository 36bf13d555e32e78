# -*- coding: utf-8 -*-
'''
Tracer particles without a GPU: the numpy restatement of the schemes, the
loss rule and the time interpolation (tests/tracer_reference.py) against
closed forms, so that the GPU tests compare against something that is itself
pinned, and every refusal of fem.Tracers (raised before the device is
touched: a Tracers of no points exists without one).
'''
import numpy
import pytest

from flow_amd import fem
from flow_amd.fem import Tracers

import point_reference as pref
import tracer_reference as tref

EMPTY = numpy.zeros((0, 2))


def test_locate_and_field_values_are_point_reference():
    '''The restatement's two short cuts give what tests/point_reference.py
    gives: the same cells, also on vertices and edges, and the same values
    (two summation orders of <= 6 products: a few ulp).'''
    for mesh in (fem.karman_channel(60, 14, fitted=True),
                 fem.karman_channel_graded(lcar=1.0e-2)):
        pts = numpy.concatenate([pref.random_points(mesh, 1500, seed=4),
                                 mesh.points[::7], pref.edge_midpoints(mesh)[::9]])
        assert len(pts) * mesh.num_cells() > 200000 or mesh.num_cells() < 400
        b = tref._buckets(mesh)
        got = tref.locate(mesh, pts)
        # (the bucket path itself, also where the brute force is the default)
        idx = b.index(pts)
        for i in range(0, len(pts), 37):
            sub = b.sub[int(idx[i, 0]), int(idx[i, 1])]
            loc = pref.locate(sub, pts[i:i + 1])[0]
            assert (sub.cells[loc] if loc >= 0 else -1) == got[i]
        assert numpy.array_equal(got, pref.locate(mesh, pts))
        for deg in (1, 2):
            V = fem.VectorFunctionSpace(mesh, 'CG', deg)
            u = tref.interpolate(V, [lambda x, y: numpy.sin(9 * x) * y + 1.0,
                                     lambda x, y: numpy.cos(7 * y) * x])
            f = numpy.nonzero(got >= 0)[0][:300]
            a = tref.field_values(u, pts[f], got[f])
            w = pref.field_values(u, pts[f], got[f])
            assert numpy.abs(a - w).max() <= 1e-14 * numpy.abs(w).max()


@pytest.mark.parametrize('sign', [1, -1])
@pytest.mark.parametrize('deg', [1, 2])
@pytest.mark.parametrize('scheme', tref.SCHEMES)
@pytest.mark.parametrize('kind', ['square', 'channel'])
def test_rigid_rotation(kind, scheme, deg, sign):
    '''x_n - c = T_k(dt J)^n (x_0 - c) for a field both spaces hold exactly;
    e_ref, the restatement's deviation, is rounding only.'''
    mesh, c, starts = tref.rotation_case(kind)
    u = tref.rotation_field(mesh, deg, c)
    dt, steps = sign * tref.ROTATION_DT, tref.ROTATION_STEPS
    pos, cells, _ = tref.advect(mesh, starts, u, dt, steps, scheme)
    want = tref.rotation_closed_form(c, starts, scheme, dt, steps)
    assert (cells >= 0).all()
    # the circles stay clear of the hole and of the walls
    r = numpy.linalg.norm(want - c, axis=1)
    assert r.max() < (0.45 if kind == 'square' else 0.055)
    assert kind == 'square' or r.min() > 0.025
    e_ref = numpy.abs(pos - want).max() / tref.diameter(mesh)
    print('rotation %-7s %-5s P%d dt %+.2f: e_ref %.2e' % (kind, scheme, deg, dt,
                                                        e_ref))
    assert e_ref < 1e-11
    assert numpy.array_equal(cells, pref.locate(mesh, pos))


def test_rigid_rotation_400_substeps():
    mesh, c, starts = tref.rotation_case('channel')
    u = tref.rotation_field(mesh, 2, c)
    pos, cells, _ = tref.advect(mesh, starts, u, 0.01, 400, 'rk4')
    want = tref.rotation_closed_form(c, starts, 'rk4', 0.01, 400)
    e_ref = numpy.abs(pos - want).max() / tref.diameter(mesh)
    print('rotation channel rk4 P2, 400 substeps: e_ref %.2e' % e_ref)
    assert (cells >= 0).all() and e_ref < 1e-11


@pytest.mark.parametrize('deg', [1, 2])
def test_time_interpolation(deg):
    '''u = (1, 0), u_next = (3, 0): RK4 and RK2 integrate a velocity linear
    in time exactly, displacement 2 steps dt; Euler sums the left values,
    1 + 2 s / steps over the substeps: steps dt (1 + (steps - 1) / steps).'''
    mesh = fem.UnitSquareMesh(12, 9)
    u0 = tref.constant_field(mesh, deg, 1.0)
    u1 = tref.constant_field(mesh, deg, 3.0)
    starts = numpy.array([[0.1, 0.3], [0.2, 0.77], [0.05, 0.5]])
    dt, steps = 0.02, 10
    for scheme in tref.SCHEMES:
        pos, cells, _ = tref.advect(mesh, starts, u0, dt, steps, scheme, u_next=u1)
        dx = 2.0 * steps * dt if scheme != 'euler' \
            else steps * dt * (1.0 + (steps - 1.0) / steps)
        assert (cells >= 0).all()
        assert numpy.abs(pos - (starts + [dx, 0.0])).max() < 1e-14
        # backwards in time
        back, cells, _ = tref.advect(mesh, starts + [0.5, 0.0], u0, -dt, steps,
                                     scheme, u_next=u1)
        assert numpy.abs(back - (starts + [0.5 - dx, 0.0])).max() < 1e-14


@pytest.mark.parametrize('deg', [1, 2])
def test_exit_exactly(deg):
    mesh = fem.UnitSquareMesh(12, 9)
    u = tref.constant_field(mesh, deg, 1.0)
    for steps in (1, 7, 8, 9, 10, 12, 13, 20):
        done, lost, want = tref.exit_prediction(steps)
        pos, cells, dist = tref.advect(mesh, tref.EXIT_STARTS, u, tref.EXIT_DT,
                                       steps, 'rk4')
        assert dist.min() > 1e-3
        assert numpy.array_equal(cells < 0, lost)
        # a live particle's cell is its position's, a lost one keeps the
        # position of the start of the substep that lost it: that of a run
        # that stops there and done * dt from the start (to an ulp, not bit
        # for bit: the sum of the P2 basis is 1 to rounding only, and numpy's
        # matrix products round differently for another number of points;
        # the device is held to the bits in tests/test_tracers_gpu.py)
        assert numpy.array_equal(cells[~lost], pref.locate(mesh, pos[~lost]))
        for i in numpy.nonzero(lost)[0]:
            stop, c, _ = tref.advect(mesh, tref.EXIT_STARTS[i:i + 1], u,
                                     tref.EXIT_DT, int(done[i]), 'rk4')
            assert c[0] >= 0 and numpy.abs(stop[0] - pos[i]).max() <= 5e-16
        assert numpy.abs(pos - want).max() < 1e-14
    assert lost.all() and numpy.array_equal(done, [12, 12, 9, 9, 7, 7])


def test_lost_from_the_start_never_move():
    mesh = fem.karman_channel(60, 14, fitted=True)
    u = tref.constant_field(mesh, 2, 1.0, 0.5)
    starts = numpy.array([[-0.1, 0.0], [mesh.hole[0], mesh.hole[1]], [0.3, 0.02]])
    pos, cells, _ = tref.advect(mesh, starts, u, 0.01, 5, 'rk2')
    assert list(cells < 0) == [True, True, False]
    assert numpy.array_equal(pos[:2], starts[:2])


def test_refusals(monkeypatch):
    mesh = fem.UnitSquareMesh(4, 4)
    other = fem.UnitSquareMesh(4, 4)
    W = fem.VectorFunctionSpace(mesh, 'CG', 2)
    W1 = fem.VectorFunctionSpace(mesh, 'CG', 1)
    u, u1 = fem.Function(W), fem.Function(W1)
    tr = Tracers(mesh, EMPTY)
    assert len(tr) == 0 and tr.positions().shape == (0, 2)
    assert tr.cells().dtype == numpy.int32 and tr.alive().dtype == bool
    # nothing to move: no device needed
    assert tr.advect(u, 0.1) is None
    assert tr.advect(u, -0.1, steps=3, scheme='euler', u_next=fem.Function(W)) is None
    assert len(tr.compact()) == 0
    scalar = fem.Function(fem.FunctionSpace(mesh, 'CG', 2))
    mixed = fem.FunctionSpace(
        mesh, fem.VectorElement('CG', 'triangle', 2)
        * fem.FiniteElement('CG', 'triangle', 1))
    for bad in (scalar, mixed, 3.0):
        with pytest.raises(ValueError):
            tr.advect(bad, 0.1)
    # (the package builds no space of another degree: a stand-in that says 3)
    class Cubic(object):
        degree, dim, component, layout = 3, 2, None, W.layout

        def mesh(self):
            return mesh

    class OnCubic(object):
        def function_space(self):
            return Cubic()

    with pytest.raises(ValueError, match='degree'):
        tr.advect(OnCubic(), 0.1)
    with pytest.raises(ValueError, match='another mesh'):
        tr.advect(fem.Function(fem.VectorFunctionSpace(other, 'CG', 2)), 0.1)
    with pytest.raises(ValueError, match='u_next'):
        tr.advect(u, 0.1, u_next=u1)
    with pytest.raises(ValueError, match='u_next'):
        tr.advect(u, 0.1, u_next=scalar)
    with pytest.raises(ValueError, match='scheme'):
        tr.advect(u, 0.1, scheme='rk3')
    for steps in (0, -2, 1.5):
        with pytest.raises(ValueError, match='steps'):
            tr.advect(u, 0.1, steps=steps)
    for dt in (float('nan'), float('inf'), -float('inf')):
        with pytest.raises(ValueError, match='dt'):
            tr.advect(u, dt)
    with pytest.raises(ValueError):
        Tracers(mesh, numpy.zeros((3, 3)))
    from flow_amd import parallel
    monkeypatch.setattr(parallel, 'active', lambda: True)
    for call in (lambda: Tracers(mesh, EMPTY), lambda: tr.advect(u, 0.1),
                 lambda: tr.inject(EMPTY), lambda: tr.evaluate(u)):
        with pytest.raises(NotImplementedError, match='on strips'):
            call()


def test_abi():
    from flow_amd import _hip
    lib = _hip.load_library()
    assert lib.flow_abi_version() == 30
    assert 'flow_advect_points' in _hip.SYMBOLS
