# -*- coding: utf-8 -*-
'''
fem.Transfer on the HIP path (flow_amd/fem/transfer.py; csrc/
transfer_kernels.hip: nearest_cells_kernel, transfer_apply_kernel) against
the numpy restatement of tests/transfer_reference.py.

The bound.  BOUND = 10 * the largest error, relative to max|u|, that the
RESTATEMENT shows against the nodal interpolant of the polynomial over all
cases of test_polynomial_reproduction (computed here from the restatement in
fp64, never from the device's result): the arithmetic is the same, only the
order of the operations differs.  The other tests use the same BOUND.

Mesh pairs.  karman_channel(24, fitted=True) does not exist (the generator's
blend-zone assertion fails below nx = 28), and between fitted channels whose
circles share their centre (30, 60, 90) no node of the finer lies outside the
coarser.  The extrapolation tests therefore take 28 -> 60 and 28 -> 48: the
reference finds 18 of 3460 P2 nodes of the finer mesh outside, all at the
cylinder, at most 6.7e-3 away where the longest obstacle edge of the source
is 1.6e-2 (asserted below from the reference, not assumed).

Every test prints its measured error next to its bound (pytest -s).
'''
import functools

import numpy
import pytest
import torch

from flow_amd import _hip, device, fem, karman
from flow_amd.fem import Transfer
import flow_amd.navier_stokes as navsto

import transfer_reference as tref

pytestmark = pytest.mark.gpu

CHANNEL = (0.0, 0.6, -0.07, 0.07)
RECT = (fem.Point(-0.3, 0.1), fem.Point(1.1, 0.9))


def _quad(x, y):
    return 1.0 + 2.0 * x - 3.0 * y + 0.5 * x * x + x * y - 2.0 * y * y


def _quad2(x, y):
    return -0.5 + x - y + 3.0 * x * x - 2.0 * x * y + y * y


def _lin(x, y):
    return 3.0 + x - 2.0 * y


def _lin2(x, y):
    return -1.0 + 0.25 * x + 4.0 * y


def _wave(x, y):
    return numpy.sin(20 * x) * y + 1.0


def _wave2(x, y):
    return numpy.cos(15 * y) * x - 0.5


def _space(mesh, deg, dim):
    return fem.FunctionSpace(mesh, 'CG', deg, dim=dim)


def _function(V, values):
    u = fem.Function(V)
    u.set_array(values)
    return u


def _polynomial_cases():
    src = fem.RectangleMesh(RECT[0], RECT[1], 7, 5, 'right')
    dst = fem.RectangleMesh(RECT[0], RECT[1], 11, 9, 'crossed')
    for deg_from, funcs in ((2, (_quad, _quad2)), (1, (_lin, _lin2))):
        for dim in (1, 2):
            for deg_to in (1, 2):
                yield (_space(src, deg_from, dim), _space(dst, deg_to, dim),
                       funcs[:dim])


@functools.lru_cache(maxsize=None)
def _bound():
    '''10 * the restatement's largest relative error on the polynomials.'''
    worst = 0.0
    for V_from, V_to, funcs in _polynomial_cases():
        want = tref.nodal(V_to, funcs)
        got = tref.transfer(V_from, V_to, tref.nodal(V_from, funcs))
        worst = max(worst, numpy.abs(got - want).max() / numpy.abs(want).max())
    assert 0.0 < worst < 1e-13
    return 10.0 * worst


def _within(got, want, what):
    err = numpy.abs(got - want).max() / numpy.abs(want).max()
    print('%s: error %.2e  bound %.2e' % (what, err, _bound()))
    assert err <= _bound()


# -- 1. same mesh ---------------------------------------------------------------
@pytest.mark.parametrize('dim', [1, 2])
@pytest.mark.parametrize('kind', ['square', 'channel'])
def test_same_mesh(hip, kind, dim):
    mesh = fem.UnitSquareMesh(12, 9) if kind == 'square' \
        else fem.karman_channel(60, 14, fitted=True)
    P1, P2 = _space(mesh, 1, dim), _space(mesh, 2, dim)
    funcs = (_wave, _wave2)[:dim]
    u1, u2 = _function(P1, tref.nodal(P1, funcs)), _function(P2, tref.nodal(P2, funcs))
    for V, u in ((P1, u1), (P2, u2)):
        T = Transfer(V, V)
        assert T.found.all() and not T.distance.any()
        w = T.apply(u)
        assert w.function_space().same_as(V) and w.data.data_ptr() != u.data.data_ptr()
        assert torch.equal(w.data, u.data)
    # P2 -> P1: the vertex dofs, bit for bit
    down = Transfer(P2, P1).apply(u2)
    a2 = u2.array().reshape(dim, P2.N)
    assert numpy.array_equal(down.array().reshape(dim, P1.N),
                             a2[:, P2.layout.vertex_dofs[numpy.argsort(P1.layout.vertex_dofs)]])
    # P1 -> P2: vertex values and exact edge means; and back: the identity
    up = Transfer(P1, P2).apply(u1)
    a1 = u1.array().reshape(dim, P1.N)
    au = up.array().reshape(dim, P2.N)
    assert numpy.array_equal(au[:, P2.layout.vertex_dofs], a1[:, P1.layout.vertex_dofs])
    e = mesh.edges
    assert numpy.array_equal(
        au[:, P2.layout.edge_dofs],
        0.5 * (a1[:, P1.layout.vertex_dofs[e[:, 0]]] + a1[:, P1.layout.vertex_dofs[e[:, 1]]]))
    assert torch.equal(Transfer(P2, P1).apply(up).data, u1.data)
    # the two public spellings
    for V_to, u, T in ((P1, u2, Transfer(P2, P1)), (P2, u1, Transfer(P1, P2)),
                       (P2, u2, Transfer(P2, P2))):
        want = T.apply(u)
        assert torch.equal(fem.interpolate(u, V_to).data, want.data)
        w = fem.Function(V_to)
        ptr = w.data.data_ptr()
        assert w.interpolate(u) is None
        assert w.data.data_ptr() == ptr and torch.equal(w.data, want.data)


def test_interpolate_constant_and_expression_as_before(hip):
    mesh = fem.UnitSquareMesh(12, 9)
    for dim, const, code in ((1, 2.5, 'sin(3*x[0])*x[1] + 1.0'),
                             (2, (1.5, -0.25), ('sin(3*x[0])*x[1]', 'x[0] - 2*x[1]'))):
        for deg in (1, 2):
            V = _space(mesh, deg, dim)
            c = fem.interpolate(fem.Constant(const), V).array().reshape(dim, V.N)
            want = numpy.repeat(numpy.atleast_1d(const)[:, None], V.N, axis=1)
            assert numpy.array_equal(c, want)
            expr = fem.Expression(code, degree=2)
            vals = expr.eval(V.layout.dof_coords.T).reshape(-1)
            assert numpy.array_equal(fem.interpolate(expr, V).array(), vals)
            w = fem.Function(V)
            w.interpolate(expr)
            assert numpy.array_equal(w.array(), vals)
            w.interpolate(fem.Constant(const))
            assert numpy.array_equal(w.array().reshape(dim, V.N), want)


# -- 2. polynomial reproduction across meshes -----------------------------------
def test_polynomial_reproduction(hip):
    for V_from, V_to, funcs in _polynomial_cases():
        T = Transfer(V_from, V_to)
        assert T.found.all() and not T.distance.any()
        tab = tref.table(V_from, V_to)
        assert tab.found.all()
        assert numpy.array_equal(T.cells, tab.cells)
        u = _function(V_from, tref.nodal(V_from, funcs))
        want = tref.nodal(V_to, funcs)
        w = T.apply(u)
        assert w.function_space().same_as(V_to)
        _within(w.array(), want, 'polynomial P%d -> P%d dim %d'
                % (V_from.degree, V_to.degree, V_to.dim))
        assert torch.equal(fem.interpolate(u, V_to).data, w.data)


# -- 3. the numpy reference on unstructured data --------------------------------
@pytest.mark.parametrize('back', [False, True])
def test_against_reference_unstructured(hip, back):
    '''The two circles differ (the structured generator moves the centre to a
    grid vertex), so each mesh has nodes inside the other's hole: with
    extrapolation, and the cells compared node for node all the same.'''
    a = fem.karman_channel(40, fitted=True)
    b = fem.karman_channel_graded(lcar=8e-3)
    src, dst = (b, a) if back else (a, b)
    for deg_from, deg_to, dim, funcs in ((2, 2, 2, (_wave, _wave2)),
                                         (1, 1, 1, (_wave,)),
                                         (2, 1, 2, (_wave, _wave2)),
                                         (1, 2, 1, (_wave,))):
        V_from, V_to = _space(src, deg_from, dim), _space(dst, deg_to, dim)
        tab = tref.table(V_from, V_to)
        T = Transfer(V_from, V_to, allow_extrapolation=True)
        assert T.cells.dtype == numpy.int32
        assert numpy.array_equal(T.cells, tab.cells)
        assert numpy.array_equal(T.found, tab.found)
        assert tab.found.mean() > 0.9
        vals = tref.nodal(V_from, funcs)
        want = tref.transfer(V_from, V_to, vals, tab)
        _within(T.apply(_function(V_from, vals)).array(), want,
                'unstructured %s P%d -> P%d dim %d (%d of %d outside)'
                % ('back' if back else 'forth', deg_from, deg_to, dim,
                   (~tab.found).sum(), len(tab.found)))


# -- 4. extrapolation ------------------------------------------------------------
def test_extrapolation(hip):
    src = fem.karman_channel(28, fitted=True)
    dst = fem.karman_channel(60, fitted=True)
    V_from, V_to = _space(src, 2, 2), _space(dst, 2, 2)
    tab = tref.table(V_from, V_to)
    out = ~tab.found
    # what the reference says about the pair: a minority at the cylinder
    share, far = out.mean(), tab.distance.max()
    obstacle = tref.obstacle_facets(src, CHANNEL)
    fa, fb = tref.facet_segments(src)
    longest = numpy.linalg.norm(fb[obstacle] - fa[obstacle], axis=1).max()
    print('outside: %d of %d (share %.2e, boundary nodes %.2e), farthest %.3e, '
          'longest obstacle edge %.3e' % (out.sum(), len(out), share,
                                          tref.boundary_node_share(V_to), far, longest))
    assert 0.0 < share < tref.boundary_node_share(V_to)
    assert numpy.isin(tab.facet[out], obstacle).all()
    assert far <= longest

    with pytest.raises(ValueError, match=r'^%d of %d target nodes' % (out.sum(), len(out))):
        Transfer(V_from, V_to)
    T = Transfer(V_from, V_to, allow_extrapolation=True)
    assert numpy.array_equal(T.found, tab.found)
    assert numpy.array_equal(T.cells, tab.cells)
    assert numpy.array_equal(T.cells[out], src.bfacet_cell[tab.facet[out]])
    assert not T.distance[~out].any()
    diam = src._edge_lengths().max(axis=1)[T.cells[out]]
    err = (numpy.abs(T.distance[out] - tab.distance[out]) / diam).max()
    print('distance: error %.2e of the cell diameter  bound %.2e' % (err, _bound()))
    assert err <= _bound()
    bary = device.to_host(T._bary).numpy()[:3 * T.n].reshape(3, T.n)
    assert (bary[src.bfacet_local[tab.facet[out]], numpy.nonzero(out)[0]] == 0.0).all()
    assert (bary[:, out] >= 0.0).all() and (bary[:, out] <= 1.0).all()
    # (the same operations in the same order: the reference's bits)
    assert numpy.array_equal(bary[:, out], tab.bary[:, out])
    vals = tref.nodal(V_from, (_wave, _wave2))
    want = tref.transfer(V_from, V_to, vals, tab)
    got = T.apply(_function(V_from, vals)).array()
    _within(got, want, 'extrapolation, all nodes')
    o2 = numpy.concatenate([out, out])
    _within(got[o2], want[o2], 'extrapolation, nodes outside')
    # a clamp: within the range of the source cell's values on that edge
    with pytest.raises(ValueError, match='max_distance'):
        Transfer(V_from, V_to, allow_extrapolation=True, max_distance=0.5 * far)
    T2 = Transfer(V_from, V_to, allow_extrapolation=True, max_distance=2.0 * far)
    assert numpy.array_equal(T2.cells, T.cells)
    # P1 targets: vertices on the finer circle
    V1 = _space(dst, 1, 2)
    tab1 = tref.table(V_from, V1)
    T1 = Transfer(V_from, V1, allow_extrapolation=True)
    assert (~tab1.found).any()
    assert numpy.array_equal(T1.cells, tab1.cells)
    assert numpy.array_equal(T1.found, tab1.found)


def test_nearest_cells_far_points(hip):
    '''flow_nearest_cells itself, on points anywhere: in the hole, outside
    the bounding box, far away; points that have a cell keep it.'''
    import ctypes
    from flow_amd.fem import ops, points, transfer
    import point_reference as pref
    mesh = fem.karman_channel(28, fitted=True)
    cx, cy, rad = mesh.hole
    pts = numpy.concatenate([
        pref.random_points(mesh, 4000, seed=8, margin=0.3),
        [[cx, cy], [5.0, 5.0], [-2.0, 0.0], [0.3, -3.0], [0.6, 0.07], [0.0, -0.07]],
        mesh.points[::5]])
    n = len(pts)
    tab = tref.Table(mesh, pts)
    assert (~tab.found).sum() > 1000 and tab.found.sum() > 1000
    probes = fem.Probes(mesh, pts)
    cell, bary = probes._cell.clone(), probes._bary.clone()
    before_bary = device.to_host(bary).numpy()[:3 * n].reshape(3, n).copy()
    dist = device.empty(n)
    gs, fc, fl, nf = transfer._facet_grid_struct(mesh)
    count = _hip.launch_count()
    _hip.check(_hip.lib().flow_nearest_cells(
        ctypes.byref(ops.mesh_struct(mesh)), ctypes.byref(gs), nf,
        _hip.i32(fc, nf), _hip.i32(fl, nf), n, _hip.f64(probes._xy, 2 * n),
        _hip.i32(cell, n), _hip.f64(bary, 3 * n), _hip.f64(dist, n), _hip.stream()))
    assert _hip.launch_count() == count + 1
    got_cell = device.to_host(cell).numpy()[:n]
    got_bary = device.to_host(bary).numpy()[:3 * n].reshape(3, n)
    got_dist = device.to_host(dist).numpy()[:n]
    assert numpy.array_equal(got_cell, tab.cells)
    f = tab.found
    assert numpy.array_equal(got_bary[:, f], before_bary[:, f])
    assert not got_dist[f].any()
    assert numpy.array_equal(got_bary[:, ~f], tab.bary[:, ~f])
    scale = numpy.maximum(tab.distance[~f], mesh.hmax())
    err = (numpy.abs(got_dist[~f] - tab.distance[~f]) / scale).max()
    print('nearest cells: distance error %.2e  bound %.2e' % (err, _bound()))
    assert err <= _bound()


# -- 5. determinism, no allocation, one launch ----------------------------------
def test_determinism_and_bookkeeping(hip):
    src = fem.karman_channel(28, fitted=True)
    dst = fem.karman_channel(60, fitted=True)
    V_from, V_to = _space(src, 2, 2), _space(dst, 2, 2)
    u = _function(V_from, tref.nodal(V_from, (_wave, _wave2)))
    Ta = Transfer(V_from, V_to, allow_extrapolation=True)
    Tb = Transfer(V_from, V_to, allow_extrapolation=True)
    assert numpy.array_equal(Ta.cells, Tb.cells)
    assert numpy.array_equal(Ta.distance, Tb.distance)
    assert torch.equal(Ta._bary, Tb._bary)
    w = fem.Function(V_to)
    ptr = w.data.data_ptr()
    count = _hip.launch_count()
    assert Ta.apply(u, out=w) is w
    assert _hip.launch_count() == count + 1
    assert w.data.data_ptr() == ptr
    first = w.array()
    for T in (Ta, Tb, Ta):
        count = _hip.launch_count()
        T.apply(u, out=w)
        assert _hip.launch_count() == count + 1
        assert w.data.data_ptr() == ptr
        assert numpy.array_equal(w.array(), first)
    assert torch.equal(Tb.apply(u).data, w.data)
    with pytest.raises(ValueError, match='out'):
        Ta.apply(u, out=fem.Function(V_from))


def test_abi_no_cell_is_nan(hip):
    '''flow_transfer_apply stays well-defined for an entry without a cell.'''
    import ctypes
    from flow_amd.fem import ops
    mesh = fem.UnitSquareMesh(4, 4)
    for deg in (1, 2):
        V = _space(mesh, deg, 2)
        u = _function(V, tref.nodal(V, (_quad, _quad2)))
        cell = device.to_device(numpy.array([0, -1, 3, mesh.num_cells()], dtype=numpy.int32))
        bary = device.to_device(numpy.full((3, 4), 1.0 / 3.0).reshape(-1))
        out = device.empty(8)
        _hip.check(_hip.lib().flow_transfer_apply(
            ctypes.byref(ops.space_struct(V.layout)), 2, 4, _hip.i32(cell, 4),
            _hip.f64(bary, 12), _hip.f64(u.data, 2 * V.N), _hip.f64(out, 8),
            _hip.stream()))
        got = device.to_host(out).numpy()[:8].reshape(2, 4)
        assert numpy.isnan(got[:, [1, 3]]).all()
        want = tref.evaluate(V, u.array(), numpy.array([0, 3]), numpy.full((3, 2), 1.0 / 3.0))
        assert numpy.abs(got[:, [0, 2]] - want).max() <= 1e-14 * numpy.abs(want).max()
        count = _hip.launch_count()
        _hip.check(_hip.lib().flow_transfer_apply(
            ctypes.byref(ops.space_struct(V.layout)), 2, 0, None, None, None, None,
            _hip.stream()))
        assert _hip.launch_count() == count


# -- 6. use: a fine run seeded from a coarse one ---------------------------------
def test_seed_a_finer_run(hip):
    from flow_amd.fem import bcs as fbcs
    coarse = karman.KarmanProblem(nx=28, scheme='ipcs')
    coarse.set_initial_profile()
    for _ in range(5):
        coarse.step()
    fine = karman.KarmanProblem(nx=48, scheme='ipcs')
    Tu = Transfer(coarse.W, fine.W, allow_extrapolation=True)
    Tp = Transfer(coarse.P, fine.P, allow_extrapolation=True)
    assert not Tu.found.all() and Tu.found.mean() > 0.99

    def first_residual(seeded):
        fine.reset(coarse.dt)
        if seeded:
            Tu.apply(coarse.u0, out=fine.u0)
            Tp.apply(coarse.p0, out=fine.p0)
            for conds, f in ((fine.u_bcs, fine.u0), (fine.p_bcs, fine.p0)):
                dofs, vals = fbcs.collect(list(conds), f.function_space().size())
                fem.ops._set_values(device.to_device(dofs), device.to_device(vals),
                                    f.data)
        fine.step(adapt=False)
        res = navsto.last_step_info['newton_residuals']
        assert numpy.isfinite(fine.u0.array()).all()
        return float(res[0])

    seeded, zero = first_residual(True), first_residual(False)
    print('first Newton residual on karman_channel(48): %.3e from the fields '
          'of karman_channel(28), %.3e from zero fields' % (seeded, zero))
    assert numpy.isfinite(seeded) and numpy.isfinite(zero)
    assert seeded < zero
