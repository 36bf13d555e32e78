# -*- coding: utf-8 -*-
'''
The adaptive loop on the HIP path (flow_amd/fem/adapt.py; csrc/
adapt_kernels.hip: jump_indicator_kernel) against the numpy evaluator of
tests/adapt_reference.py.

The bound.  max |eta2_gpu - eta2_ref| <= 1e-12 * max(eta2_ref): both sides
are fp64 sums of a few hundred operations in different orders, about 4e3 ulps
of the largest term; nodal values are random in [-1, 1], so the jumps are as
large as the gradients and nothing cancels.

Meshes.  Every karman_channel_graded builds, down to 18 cells; the one here
(lcar 0.006, 583 cells, three blocks) is the coarsest with more than two
blocks.  Its Delaunay cells are all listed counter-clockwise and meet in
seven of the nine pairings of local facets only, so 'graded' here is that
mesh with every cell's vertex list turned and mirrored at random (seeded):
all nine pairings, both directions, cells of both orientations.

Every test prints its measured error next to its bound (pytest -s).
'''
import functools
import math

import numpy
import pytest
import torch

from flow_amd import device, fem
from flow_amd.fem import JumpIndicator, Transfer, mark, refine

import adapt_reference as aref

pytestmark = pytest.mark.gpu

TOL = 1e-12


@functools.lru_cache(maxsize=None)
def _mesh(name):
    if name == 'tail':
        return fem.UnitSquareMesh(5, 4)                 # 40 cells: tail lanes
    if name.startswith('blocks '):
        return fem.UnitSquareMesh(17, 15, name[7:])     # 510: several blocks
    if name == 'hole':
        return fem.rectangle_with_hole(0.0, 1.0, 0.0, 0.5, (0.4, 0.25), 0.12,
                                       12, 6)
    assert name == 'graded'
    mesh = fem.karman_channel_graded(0.006)
    rng = numpy.random.RandomState(9)
    nc = mesh.num_cells()
    turn = (rng.randint(0, 3, nc)[:, None] + numpy.arange(3)[None, :]) % 3
    mirror = rng.uniform(size=nc) < 0.5
    turn[mirror] = turn[mirror][:, ::-1]
    cells = mesh.cell_vertices[numpy.arange(nc)[:, None], turn]
    return fem.Mesh(mesh.points, cells)


MESHES = ('tail',) + tuple('blocks ' + d for d in aref.DIAGONALS) + ('hole', 'graded')


@functools.lru_cache(maxsize=None)
def _case(name, deg, dim):
    '''(u, reference eta2) with seeded random nodal values, computed once.'''
    V = fem.FunctionSpace(_mesh(name), 'CG', deg, dim=dim)
    rng = numpy.random.RandomState(100 * deg + dim)
    u = fem.Function(V)
    u.set_array(rng.uniform(-1.0, 1.0, V.size()))
    want = aref.indicator(u)
    want.flags.writeable = False
    return u, want


def _close(got, want, what, scale=None):
    scale = numpy.abs(want).max() if scale is None else scale
    err = numpy.abs(got - want).max()
    print('%s: error %.2e  bound %.2e' % (what, err, TOL * scale))
    assert numpy.isfinite(got).all()
    assert err <= TOL * scale


# -- 1. against the reference -----------------------------------------------------
@pytest.mark.parametrize('dim', [1, 2])
@pytest.mark.parametrize('deg', [1, 2])
@pytest.mark.parametrize('name', MESHES)
def test_indicator_against_reference(hip, name, deg, dim):
    u, want = _case(name, deg, dim)
    J = JumpIndicator(u.function_space())
    eta2 = J.apply(u)
    assert eta2.dtype == torch.float64 and eta2.is_cuda
    assert tuple(eta2.shape) == (_mesh(name).num_cells(),)
    _close(device.to_host(eta2).numpy(), want, '%s P%d x%d' % (name, deg, dim))


def test_graded_mesh_pairs_every_local_facet():
    t = fem.adapt.facet_table(_mesh('graded')).reshape(3, -1)
    i = numpy.nonzero(t >= 0)[0]
    j = (t[t >= 0] >> 1) & 3
    assert len(set(zip(i.tolist(), j.tolist()))) == 9
    assert set((t[t >= 0] & 1).tolist()) == {0, 1}


@pytest.mark.parametrize('deg', [1, 2])
def test_two_cells_share_one_term(hip, deg):
    '''Only the shared edge counts: both cells get its term (each from its
    own side, so equal up to rounding), and nothing from their boundary
    edges.'''
    mesh = fem.Mesh(numpy.array([[0.0, 0.0], [1.0, 0.1], [1.2, 1.0], [-0.1, 0.8]]),
                    numpy.array([[0, 1, 2], [0, 3, 2]], dtype=numpy.int32))
    V = fem.FunctionSpace(mesh, 'CG', deg, dim=2)
    u = fem.Function(V)
    u.set_array(numpy.random.RandomState(5).uniform(-1.0, 1.0, V.size()))
    want = aref.indicator(u)
    assert want[0] == want[1] > 0.0
    got = device.to_host(fem.jump_indicator(u)).numpy()
    _close(got, want, 'two cells P%d' % deg)


# -- 2. closed forms and properties -----------------------------------------------
def test_kink_on_the_device(hip):
    mesh = fem.UnitSquareMesh(4, 4)
    u = aref.field(fem.FunctionSpace(mesh, 'CG', 1),
               [lambda x, y: numpy.abs(x - 0.5)])
    got = device.to_host(JumpIndicator(u.function_space()).apply(u)).numpy()
    want = aref.kink_expectation(mesh)
    print('kink: on the line %.2e off it %.2e'
          % (numpy.abs(got - want)[want > 0].max(), numpy.abs(got[want == 0]).max()))
    assert numpy.abs(got - want)[want > 0].max() <= 1e-15
    assert numpy.abs(got[want == 0]).max() <= 1e-28


def test_smooth_fields_have_no_jump_on_the_device(hip):
    mesh = fem.UnitSquareMesh(4, 4, 'crossed')
    for deg, dim, funcs, gmax in aref.SMOOTH:
        u = aref.field(fem.FunctionSpace(mesh, 'CG', deg, dim=dim), funcs)
        got = device.to_host(fem.jump_indicator(u)).numpy()
        print('P%d x%d smooth: %.2e  bound %.2e'
              % (deg, dim, numpy.abs(got).max(), 1e-24 * gmax**2))
        assert numpy.abs(got).max() <= 1e-24 * gmax**2


def test_apply_twice_out_and_estimate(hip):
    u, want = _case('blocks crossed', 2, 2)
    J = JumpIndicator(u.function_space())
    a = J.apply(u)
    b = J.apply(u)
    assert a.data_ptr() != b.data_ptr() and torch.equal(a, b)
    out = device.empty(len(want))
    out.fill_(-1.0)
    back = J.apply(u, out=out)
    assert back is out and torch.equal(out, a)
    with pytest.raises(ValueError, match='out'):
        J.apply(u, out=device.empty(len(want) + 1))
    est = J.estimate(u)
    ref = math.sqrt(want.sum())
    print('estimate %.15e reference %.15e' % (est, ref))
    assert isinstance(est, float) and abs(est - ref) <= 1e-12 * ref
    # the table is uploaded once per mesh
    assert JumpIndicator(u.function_space()).apply(u).data_ptr() != a.data_ptr()
    assert len(u.function_space().mesh()._cache['facet_table_dev']) == 1


# -- 3. mark ------------------------------------------------------------------------
def test_mark_on_the_device(hip):
    rng = numpy.random.RandomState(2)
    eta = rng.permutation(1000).astype(float) + 1.0     # distinct, exact sums
    dev = device.to_device(eta)
    for strategy in fem.adapt.STRATEGIES:
        for fraction in (0.05, 0.5, 1.0):
            got = mark(dev, fraction, strategy)
            assert got.dtype == bool and isinstance(got, numpy.ndarray)
            assert numpy.array_equal(got, mark(eta, fraction, strategy))
    bad = device.to_device(numpy.array([1.0, float('nan'), 2.0]))
    with pytest.raises(ValueError, match='NaN'):
        mark(bad, 0.5)


# -- 4. the adaptive loop -------------------------------------------------------------
def _device_solve(mesh, start=None):
    '''(V, nodal values, the Function) of the Poisson problem by
    solve(a == L), from `start` (a Function on another mesh) transferred.'''
    V, a, L, bcs = aref.poisson(mesh)
    uh = fem.Function(V)
    if start is not None:
        Transfer(start.function_space(), V).apply(start, out=uh)
    fem.solve(a == L, uh, bcs, solver_parameters={
        'krylov_solver': {'relative_tolerance': 1e-10}})
    return V, uh.array(), uh


def test_adaptive_loop_beats_uniform_refinement(hip):
    '''The condition of the host loop (tests/test_adapt_host.py), with the
    same SIGMA, FRACTION and CYCLES, through solve(a == L), JumpIndicator,
    mark and refine, the previous solution transferred as the start.'''
    mesh = fem.UnitSquareMesh(8, 8)
    rows, uh = [], None
    for cycle in range(aref.CYCLES + 1):
        V, x, uh = _device_solve(mesh, uh)
        rows.append((V.N, aref.l2_error(V, x)))
        if cycle == aref.CYCLES:
            break
        eta2 = JumpIndicator(V).apply(uh)
        mesh = refine(mesh, mark(eta2, aref.FRACTION, 'dorfler'))
    uniform = aref.uniform_errors(lambda m: _device_solve(m)[:2], rows[-1][0],
                                  fem.UnitSquareMesh(8, 8))
    print('adaptive: %s' % rows)
    print('uniform:  %s' % uniform)
    n, e = aref.uniform_error_for(rows[-1][0], uniform)
    assert n >= rows[-1][0]
    assert rows[-1][1] < e


# -- 5. a refined Karman mesh ---------------------------------------------------------
def _wave(x, y):
    return numpy.sin(20 * x) * y + 1.0


def _wave2(x, y):
    return numpy.cos(15 * y) * x - 0.5


def test_refined_karman_mesh_takes_the_fields(hip):
    src = fem.karman_channel(28, fitted=True)
    W = fem.VectorFunctionSpace(src, 'CG', 2)
    Q = fem.FunctionSpace(src, 'CG', 1)
    u, p = aref.field(W, [_wave, _wave2]), aref.field(Q, [_wave])
    marked = mark(JumpIndicator(W).apply(u), 0.5)
    # the cells at the obstacle as well: the hole's edges are split
    cx, cy, rad = src.hole
    cen = src.points[src.cell_vertices].mean(axis=1)
    marked |= numpy.hypot(cen[:, 0] - cx, cen[:, 1] - cy) < 1.5 * rad
    dst = refine(src, marked)
    assert dst.num_cells() > src.num_cells() and dst.hole == src.hole
    # the largest sagitta of the source polygon, from its hole edges
    ends = src.points[src.edges[src.bfacets]]
    dist = numpy.hypot(ends[:, :, 0] - cx, ends[:, :, 1] - cy)
    hole = (numpy.abs(dist - rad) <= 1e-9 * rad).all(axis=1)
    chord = numpy.hypot(*(ends[hole, 0] - ends[hole, 1]).T)
    sides = math.pi / numpy.arcsin(chord / (2.0 * rad))         # n_sides_local
    sagitta = float((rad * (1.0 - numpy.cos(math.pi / sides))).max())
    assert hole.sum() >= 8 and 0.0 < sagitta < 0.2 * rad
    for V_from, f in ((W, u), (Q, p)):
        V_to = fem.FunctionSpace(dst, 'CG', V_from.degree, dim=V_from.dim)
        T = Transfer(V_from, V_to, allow_extrapolation=True)
        # a midpoint moved onto the circle lies one sagitta from its chord,
        # give or take the 1e-12 * radius within which it is on the circle
        # (the channel lies OUTSIDE the circle: the move goes into the
        # source mesh, and the nodes on the new chords lie in it too, so no
        # node is expected outside at all)
        print('P%d: %d of %d nodes outside, farthest %.6e, largest sagitta '
              '%.6e' % (V_from.degree, (~T.found).sum(), T.n,
                        T.distance.max(), sagitta))
        assert T.distance.max() <= sagitta + 1e-12 * rad
        w = T.apply(f)
        # target nodes that are source nodes
        where = {tuple(q): k for k, q in enumerate(V_from.layout.dof_coords)}
        pairs = [(k, where[tuple(q)])
                 for k, q in enumerate(V_to.layout.dof_coords)
                 if tuple(q) in where]
        to, frm = numpy.array(pairs).T
        assert len(to) >= src.num_vertices()
        a = w.array().reshape(V_to.dim, -1)[:, to]
        b = f.array().reshape(V_from.dim, -1)[:, frm]
        err = numpy.abs(a - b).max() / numpy.abs(b).max()
        print('P%d: %d shared nodes, error %.2e' % (V_from.degree, len(to), err))
        assert err <= 1e-13
