# -*- coding: utf-8 -*-
'''
Contour lines on the HIP path (flow_amd/fem/isolines.py; csrc/
isoline_kernels.hip) against the numpy restatement of tests/
isolines_reference.py.

Meshes: UnitSquareMesh(5, 4, 'crossed') (80 cells: less than one block),
UnitSquareMesh(12, 11) (264 cells: the last block is partial and the scan
crosses a block boundary) and the small rectangle_with_hole of the host tests.
P1 and P2 on each; the field is sin(3x) cos(2y) as nodal values, five levels.

The bound on the end points, 1e-12 * the mesh's diameter.  A crossing is
x_a + t (x_b - x_a), t = (c - f_a) / (f_b - f_a): the relative error of t is
about eps * max(|f|, |c|) / |f_b - f_a|.  Every case asserts, on the
restatement, that each crossed sub-edge has |f_b - f_a| >= 1e-3 max|f|, so t is
good to about 1e-13 and the point to 1e-13 diameters; one order is left for the
contraction the two sides may differ in.  Lengths and areas are sums of at
most 4 nc positive terms added in another order: 1e-12 relative.

Every test prints what it measured next to its bound (pytest -s).
'''
import ctypes
import functools
import importlib

import numpy
import pytest
import torch

from flow_amd import _hip, device, fem
from flow_amd.fem import ops

import isolines_reference as iref
from isolines_reference import A, clip_square, hole_mesh, nodal, quarter_circle_errors
from isolines_reference import QUARTER_CIRCLE_MARGIN as MARGIN

fiso = importlib.import_module('flow_amd.fem.isolines')

pytestmark = pytest.mark.gpu

TOL = 1e-12
MESHES = ('crossed 5x4', 'square 12x11', 'hole')


@functools.lru_cache(maxsize=None)
def _mesh(name):
    if name == 'hole':
        return hole_mesh()
    if name == 'crossed 5x4':
        return fem.UnitSquareMesh(5, 4, 'crossed')
    return fem.UnitSquareMesh(12, 11)


def _wave(x, y):
    return numpy.sin(3 * x) * numpy.cos(2 * y)


class Case(object):
    '''A space, nodal values, levels and what the restatement makes of them,
    computed once and left unchanged.'''

    def __init__(self, V, values, levels):
        self.V, self.values = V, values
        self.levels = numpy.atleast_1d(numpy.asarray(levels, dtype=float))
        self.tri = iref.Triangulation(V.layout)
        self.seg = iref.segments(V.layout, values, self.levels, self.tri)
        self.length = iref.length(V.layout, values, self.levels, self.tri)
        self.area = iref.area(V.layout, values, self.levels, self.tri)
        for a in (values, self.levels, self.length, self.area) \
                + tuple(v for v in self.seg.values() if isinstance(v, numpy.ndarray)):
            a.flags.writeable = False

    def function(self):
        f = fem.Function(self.V)
        f.set_array(numpy.array(self.values))
        return f


@functools.lru_cache(maxsize=None)
def _case(name, deg):
    V = fem.FunctionSpace(_mesh(name), 'CG', deg)
    f = nodal(V, _wave)
    return Case(V, f, numpy.linspace(f.min(), f.max(), 7)[1:-1])


def host(t):
    return device.to_host(t).numpy()


def check_segments(C, case, bound):
    '''The Contours C against the restatement's segments; the largest
    distance between end points.'''
    want = case.seg
    assert C.nseg == len(want['cell'])
    assert numpy.array_equal(host(C.cell), want['cell'])
    assert numpy.array_equal(host(C.level), want['level'])
    assert numpy.array_equal(host(C.keys), want['keys'])
    xy = host(C.xy)
    assert xy.shape == (C.nseg, 4) and host(C.bary).shape == (C.nseg, 2, 3)
    err = numpy.abs(xy - want['xy']).max() if C.nseg else 0.0
    assert err <= bound
    return err


# -- 1. segments against the restatement ---------------------------------------------
@pytest.mark.parametrize('deg', [1, 2])
@pytest.mark.parametrize('name', MESHES)
def test_segments_against_reference(hip, name, deg):
    case = _case(name, deg)
    gap, top = case.seg['gap'], numpy.abs(case.values).max()
    assert gap >= 1e-3 * top, (gap, top)
    C = fem.Isolines(case.V).extract(case.function(), case.levels)
    bound = TOL * iref.diameter(case.V.mesh())
    err = check_segments(C, case, bound)
    print('%s P%d: %d cells, %d segments, smallest |f_b - f_a| %.2e max|f|, '
          'end points %.2e  bound %.2e'
          % (name, deg, case.V.mesh().num_cells(), C.nseg, gap / top, err, bound))
    assert C.nseg > 0 and set(host(C.level)) == set(range(5))
    assert C.xy.dtype == C.bary.dtype == torch.float64
    assert C.level.dtype == C.cell.dtype == C.keys.dtype == torch.int32
    # the barycentric coordinates name the same points
    P = case.V.mesh().points[case.V.mesh().cell_vertices[host(C.cell)]]
    at = numpy.einsum('sek,skd->sed', host(C.bary), P).reshape(-1, 4)
    assert numpy.abs(at - host(C.xy)).max() <= 1e-14 * iref.diameter(case.V.mesh())
    assert numpy.abs(host(C.bary).sum(axis=2) - 1.0).max() <= 1e-14
    # the one-off spelling
    D = fem.isolines(case.function(), case.levels)
    assert torch.equal(D.xy, C.xy) and torch.equal(D.keys, C.keys)


# -- 2. two calls give the same bits -------------------------------------------------
@pytest.mark.parametrize('deg', [1, 2])
@pytest.mark.parametrize('name', ['square 12x11', 'hole'])
def test_same_bits_twice(hip, name, deg):
    case = _case(name, deg)
    I, f = fem.Isolines(case.V), case.function()
    a, b = I.extract(f, case.levels), I.extract(f, case.levels)
    assert a.xy.data_ptr() != b.xy.data_ptr()
    for key in ('xy', 'keys', 'bary', 'level', 'cell'):
        assert torch.equal(getattr(a, key), getattr(b, key)), key
    assert numpy.array_equal(I.length(f, case.levels), I.length(f, case.levels))
    assert numpy.array_equal(I.area(f, case.levels), I.area(f, case.levels))


# -- 3. length and area --------------------------------------------------------------
@pytest.mark.parametrize('deg', [1, 2])
@pytest.mark.parametrize('name', MESHES)
def test_length_and_area_against_reference(hip, name, deg):
    case = _case(name, deg)
    I, f = fem.Isolines(case.V), case.function()
    length, area = I.length(f, case.levels), I.area(f, case.levels)
    assert length.shape == area.shape == (5,)
    el = numpy.abs(length / case.length - 1.0).max()
    ea = numpy.abs(area / case.area - 1.0).max()
    print('%s P%d: length %.2e, area %.2e relative  bound %.0e' % (name, deg, el, ea, TOL))
    assert el <= TOL and ea <= TOL
    # a single level is the float spelling
    assert I.length(f, float(case.levels[2]))[0] == length[2]
    # the mesh's area, and nothing
    total = case.V.mesh().cell_areas().sum()
    assert abs(I.area(f, -1e300)[0] / total - 1.0) <= TOL
    assert I.area(f, 1e300)[0] == 0.0 and I.length(f, [-1e300, 1e300]).tolist() == [0, 0]


@pytest.mark.parametrize('deg', [1, 2])
def test_linear_field_is_measured_exactly(hip, deg):
    V = fem.FunctionSpace(_mesh('crossed 5x4'), 'CG', deg)
    f = fem.Function(V)
    f.set_array(nodal(V, lambda x, y: A[0] * x + A[1] * y))
    levels = [-0.2531, 0.0123, 0.1017, 0.3313, 0.5509]
    I = fem.Isolines(V)
    C = I.extract(f, levels)
    xy, lev = host(C.xy), numpy.array(levels)[host(C.level)]
    for end in (xy[:, 0:2], xy[:, 2:4]):
        assert numpy.abs(end @ A - lev).max() <= 1e-14
    d = xy[:, 2:4] - xy[:, 0:2]
    assert ((d @ numpy.array([-A[1], A[0]])) < 0.0).all()
    want = numpy.array([clip_square(A, c) for c in levels])
    length, area = I.length(f, levels), I.area(f, levels)
    print('P%d: length %.2e, area %.2e  bound 1e-13'
          % (deg, numpy.abs(length - want[:, 0]).max(), numpy.abs(area - want[:, 1]).max()))
    assert numpy.abs(length - want[:, 0]).max() <= 1e-13
    assert numpy.abs(area - want[:, 1]).max() <= 1e-13


def test_position_converges_on_the_quarter_circle(hip):
    '''The inequality of the host test, on the device.'''
    def length_of(V, values, c):
        f = fem.Function(V)
        f.set_array(values)
        return fem.Isolines(V).length(f, c)[0]
    errs = quarter_circle_errors(length_of)
    print('P2: %.6e -> %.6e, ratio %.4f (asked: %.4f)'
          % (errs[0], errs[1], errs[0] / errs[1], MARGIN))
    assert errs[1] < errs[0] / MARGIN


# -- 4. non-finite entries -----------------------------------------------------------
@pytest.mark.parametrize('deg', [1, 2])
def test_non_finite_values_emit_nothing(hip, deg):
    base = _case('square 12x11', deg)
    values = numpy.array(base.values)
    bad = numpy.arange(7, base.V.N, 23)
    values[bad] = numpy.inf
    values[bad[1]] = -numpy.inf
    values[bad[3]] = numpy.nan
    case = Case(base.V, values, base.levels)
    assert 0 < len(case.seg['cell']) < len(base.seg['cell'])
    I, f = fem.Isolines(case.V), case.function()
    C = I.extract(f, case.levels)
    check_segments(C, case, TOL * iref.diameter(case.V.mesh()))
    assert not numpy.isin(host(C.keys), bad).any()
    assert numpy.isfinite(host(C.xy)).all() and numpy.isfinite(host(C.bary)).all()
    length, area = I.length(f, case.levels), I.area(f, case.levels)
    assert numpy.isfinite(length).all() and numpy.isfinite(area).all()
    assert numpy.abs(length / case.length - 1.0).max() <= TOL
    assert numpy.abs(area / case.area - 1.0).max() <= TOL
    assert (area < base.area).all()


# -- 5. ties and empties -------------------------------------------------------------
@pytest.mark.parametrize('deg', [1, 2])
def test_nodes_on_the_level(hip, deg):
    V = fem.FunctionSpace(_mesh('crossed 5x4'), 'CG', deg)
    case = Case(V, nodal(V, lambda x, y: numpy.round(4 * x) + numpy.round(4 * y)),
                numpy.arange(0.0, 10.0))
    I, f = fem.Isolines(V), case.function()
    C = I.extract(f, case.levels)
    # |f_b - f_a| >= 1 on a crossed sub-edge of an integer field
    assert case.seg['gap'] >= 1.0
    check_segments(C, case, TOL * iref.diameter(V.mesh()))
    xy = host(C.xy)
    assert numpy.hypot(xy[:, 2] - xy[:, 0], xy[:, 3] - xy[:, 1]).min() > 1e-3
    rows = numpy.column_stack([host(C.level), host(C.keys)])
    assert len(numpy.unique(rows, axis=0)) == len(rows)
    assert numpy.abs(I.length(f, case.levels) - case.length).max() <= TOL
    assert numpy.abs(I.area(f, case.levels) - case.area).max() <= TOL


@pytest.mark.parametrize('deg', [1, 2])
def test_no_segment_allocates_and_emits_nothing(hip, deg):
    case = _case('square 12x11', deg)
    I = fem.Isolines(case.V)
    const = fem.Function(case.V)
    const.set_array(numpy.full(case.V.N, 0.25))
    for f, levels in ((const, 0.25), (const, [0.25, 0.25]),
                      (case.function(), [-2.0, 1.5]), (const, numpy.full(40, 0.25))):
        launches = _hip.launch_count()
        C = I.extract(f, levels)
        counted = -(-len(numpy.atleast_1d(levels)) // 32)
        assert _hip.launch_count() == launches + counted     # the counts alone
        assert C.nseg == 0
        for t, shape in ((C.xy, (0, 4)), (C.level, (0,)), (C.cell, (0,)),
                         (C.keys, (0, 4)), (C.bary, (0, 2, 3))):
            assert tuple(t.shape) == shape and t.is_cuda
            assert t.untyped_storage().nbytes() == 0
        assert C.polylines() == [[] for _ in numpy.atleast_1d(levels)]
        assert tuple(C.evaluate(const).shape) == (1, 0)
        assert (I.length(f, levels) == 0.0).all()
    assert abs(I.area(const, 0.25)[0] - 1.0) <= TOL and I.area(const, 0.26)[0] == 0.0


# -- 6. more levels than one launch takes --------------------------------------------
@pytest.mark.parametrize('deg', [1, 2])
def test_33_levels_are_two_launches(hip, deg):
    case = _case('square 12x11', deg)
    I, f = fem.Isolines(case.V), case.function()
    lo, hi = case.values.min(), case.values.max()
    levels = numpy.linspace(lo, hi, 35)[1:-1]
    assert len(levels) == 33
    launches = _hip.launch_count()
    C = I.extract(f, levels)
    assert _hip.launch_count() == launches + 4               # 2 counts, 2 emits
    cell, level = host(C.cell).astype(numpy.int64), host(C.level).astype(numpy.int64)
    order = cell * 33 + level
    assert (numpy.diff(order) >= 0).all() and set(level) == set(range(33))
    length, area = I.length(f, levels), I.area(f, levels)
    for k in range(33):
        one = I.extract(f, levels[k])
        sel = torch.nonzero(C.level == k)[:, 0]
        assert one.nseg == len(sel) > 0
        for key in ('xy', 'keys', 'bary', 'cell'):
            assert torch.equal(getattr(C, key)[sel], getattr(one, key)), (k, key)
        assert I.length(f, levels[k])[0] == length[k]
        assert I.area(f, levels[k])[0] == area[k]
    want = Case(case.V, case.values, levels)
    check_segments(C, want, TOL * iref.diameter(case.V.mesh()))


# -- 7. expressions on the contour ---------------------------------------------------
@pytest.mark.parametrize('deg', [1, 2])
@pytest.mark.parametrize('name', ['square 12x11', 'hole'])
def test_evaluate_on_the_segments(hip, name, deg):
    case = _case(name, deg)
    mesh = case.V.mesh()
    f = case.function()
    C = fem.Isolines(case.V).extract(f, case.levels)
    xy = host(C.xy)
    x = fem.SpatialCoordinate(mesh)
    bound = 1e-14 * iref.diameter(mesh)
    for t, want in ((0.0, xy[:, 0:2]), (1.0, xy[:, 2:4]),
                    (0.5, 0.5 * (xy[:, 0:2] + xy[:, 2:4]))):
        got = host(C.evaluate(x, t=t))
        assert got.shape == (2, C.nseg)
        err = numpy.abs(got.T - want).max()
        print('%s P%d t=%g: |x - x(t)| max %.2e  bound %.2e' % (name, deg, t, err, bound))
        assert err <= bound
    assert torch.equal(C.evaluate(x), C.evaluate(x, t=0.5))
    if deg == 1:
        # linear along the segment: the level, wherever
        lev = case.levels[host(C.level)]
        top = numpy.abs(case.values).max()
        for t in (0.0, 0.3, 1.0):
            got = host(C.evaluate(f, t=t))
            assert got.shape == (1, C.nseg)
            err = numpy.abs(got[0] - lev).max()
            print('%s: |f - c| max %.2e at t=%g  bound %.2e' % (name, err, t, 1e-13 * top))
            assert err <= 1e-13 * top


# -- 8. polylines --------------------------------------------------------------------
@pytest.mark.parametrize('deg', [1, 2])
def test_polylines_on_the_hole_mesh(hip, deg):
    case = _case('hole', deg)
    I, f = fem.Isolines(case.V), case.function()
    C = I.extract(f, case.levels)
    boundary = case.tri.boundary_keys()
    keys, level, xy = host(C.keys), host(C.level), host(C.xy)
    chains = fiso.chain_segments(keys, level, 5)
    lines = C.polylines()
    assert len(lines) == len(chains) == 5 and C.polylines(3)[0][0].shape[1] == 2
    summed = numpy.zeros(5)
    for k in range(5):
        assert len(lines[k]) == len(chains[k]) > 0
        assert sum(len(idx) for idx, _ in chains[k]) == (level == k).sum()
        for (pts, closed), (idx, flag) in zip(lines[k], chains[k]):
            assert closed == flag and len(pts) == len(idx) + (not closed)
            assert (level[idx] == k).all()
            assert (keys[idx[1:], 0:2] == keys[idx[:-1], 2:4]).all()
            assert numpy.array_equal(pts[:len(idx)], xy[idx, 0:2])
            if closed:
                assert tuple(keys[idx[-1], 2:4]) == tuple(keys[idx[0], 0:2])
                ring = numpy.concatenate([pts, pts[:1]])
            else:
                assert tuple(keys[idx[0], 0:2]) in boundary
                assert tuple(keys[idx[-1], 2:4]) in boundary
                ring = pts
            # consecutive segments meet bit for bit
            assert numpy.array_equal(xy[idx[1:], 0:2], xy[idx[:-1], 2:4])
            step = numpy.diff(ring, axis=0)
            summed[k] += numpy.hypot(step[:, 0], step[:, 1]).sum()
    length = I.length(f, case.levels)
    print('P%d: %s lines; sum of segments against length: %.2e relative'
          % (deg, [len(l) for l in lines], numpy.abs(summed / length - 1.0).max()))
    assert numpy.abs(summed / length - 1.0).max() <= TOL


# -- 9. the entry points refuse what they cannot run ---------------------------------
def test_argument_errors_launch_nothing_and_capacity_cuts_the_tail(hip):
    case = _case('square 12x11', 2)
    V = case.V
    nc = V.mesh().num_cells()
    mesh_s, space_s = ops.mesh_struct(V.mesh()), ops.space_struct(V.layout)
    f = case.function()
    fp = _hip.f64(f.data, V.N)
    lev = fiso._launches(case.levels)[0]
    dev = device.get()
    count = torch.zeros(nc, dtype=torch.int32, device=dev)
    st = _hip.stream()
    m, s, L = ctypes.byref(mesh_s), ctypes.byref(space_s), ctypes.byref(lev)
    pc = _hip.i32(count, nc)
    total = len(case.seg['cell'])
    full = fem.Isolines(V).extract(f, case.levels)
    assert full.nseg == total

    def outputs(n):
        t = (torch.full((n, 4), -7.0, dtype=torch.float64, device=dev),
             torch.full((n,), -7, dtype=torch.int32, device=dev),
             torch.full((n,), -7, dtype=torch.int32, device=dev),
             torch.full((n, 4), -7, dtype=torch.int32, device=dev),
             torch.full((n, 2, 3), -7.0, dtype=torch.float64, device=dev))
        p = [_hip.f64(t[0]), _hip.i32(t[1]), _hip.i32(t[2]), _hip.i32(t[3]),
             _hip.f64(t[4])]
        return t, p

    out, po = outputs(total)
    work, res = device.empty(2 * 32 * 2), device.empty(64)
    pw, pr = _hip.f64(work), _hip.f64(res)
    launches = _hip.launch_count()
    strips = _hip.MeshS.from_buffer_copy(mesh_s)
    strips.c1 = 1
    many = _hip.IsolineLevels(33, 0)
    for mm, ss, ff, LL in ((None, s, fp, L), (m, None, fp, L), (m, s, None, L),
                           (m, s, fp, None), (ctypes.byref(strips), s, fp, L),
                           (m, s, fp, ctypes.byref(many))):
        assert hip.flow_isoline_count(mm, ss, ff, LL, pc, st) == 2
        assert hip.flow_isoline_emit(mm, ss, ff, LL, pc, pc, total, *po, st) == 2
        assert hip.flow_isoline_measure(mm, ss, ff, LL, pw, pr, st) == 2
    assert hip.flow_isoline_count(m, s, fp, L, None, st) == 2
    assert hip.flow_isoline_emit(m, s, fp, L, None, pc, total, *po, st) == 2
    assert hip.flow_isoline_emit(m, s, fp, L, pc, None, total, *po, st) == 2
    for k in range(5):
        args = list(po)
        args[k] = None
        assert hip.flow_isoline_emit(m, s, fp, L, pc, pc, total, *args, st) == 2
    assert hip.flow_isoline_measure(m, s, fp, L, None, pr, st) == 2
    assert hip.flow_isoline_measure(m, s, fp, L, pw, None, st) == 2
    with pytest.raises(ValueError, match='invalid argument'):
        _hip.check(2)
    none = _hip.IsolineLevels(0, 0)
    N = ctypes.byref(none)
    assert hip.flow_isoline_count(m, s, fp, N, pc, st) == 0
    assert hip.flow_isoline_emit(m, s, fp, N, pc, pc, total, *po, st) == 0
    assert hip.flow_isoline_measure(m, s, fp, N, pw, pr, st) == 0
    assert hip.flow_isoline_emit(m, s, fp, L, pc, pc, 0, *po, st) == 0
    assert _hip.launch_count() == launches
    # ... and run what they can: the count, the caller's scan, an emit that is
    # given room for the first `room` segments only
    _hip.check(hip.flow_isoline_count(m, s, fp, L, pc, st))
    assert _hip.launch_count() == launches + 1
    got = host(count).astype(numpy.int64)
    assert numpy.array_equal(got, numpy.bincount(case.seg['cell'], minlength=nc))
    offset = torch.from_numpy((numpy.cumsum(got) - got).astype(numpy.int32)).to(dev)
    room = total // 2
    assert 0 < room < total
    _hip.check(hip.flow_isoline_emit(m, s, fp, L, pc, _hip.i32(offset, nc), room, *po, st))
    assert _hip.launch_count() == launches + 2
    for t, want in zip(out, (full.xy, full.level, full.cell, full.keys, full.bary)):
        assert torch.equal(t[:room], want[:room])
        assert (host(t[room:]) == -7).all()


def test_a_cell_that_names_no_dof_of_the_space(hip):
    '''A copy of cell_dofs with two entries outside [0, n), passed straight
    to the entry points: those cells count one record each, filled with NaN
    and -1; every other cell is what the restatement says.  (The kernels
    test a dof against [0, n) before they use it as an index and read
    f[0] instead: load_values in csrc/isoline_kernels.hip.)'''
    case = _case('square 12x11', 2)
    V = case.V
    nc = V.mesh().num_cells()
    cd = numpy.array(V.layout.cell_dofs.T, dtype=numpy.int32)       # (nloc, nc)
    broken = (5, 260)
    cd[4, broken[0]] = V.N
    cd[0, broken[1]] = -1
    cd_dev = device.to_device(cd)
    space_s = _hip.SpaceS.from_buffer_copy(ops.space_struct(V.layout))
    space_s.cell_dofs = _hip.i32(cd_dev, 6 * nc).value
    mesh_s = ops.mesh_struct(V.mesh())
    f = case.function()
    fp = _hip.f64(f.data, V.N)
    lev = fiso._launches(case.levels)[0]
    dev = device.get()
    m, s, L = ctypes.byref(mesh_s), ctypes.byref(space_s), ctypes.byref(lev)
    st = _hip.stream()
    count = torch.zeros(nc, dtype=torch.int32, device=dev)
    _hip.check(hip.flow_isoline_count(m, s, fp, L, _hip.i32(count, nc), st))
    got = host(count).astype(numpy.int64)
    want = numpy.bincount(case.seg['cell'], minlength=nc)
    want[list(broken)] = 1
    assert numpy.array_equal(got, want)
    total = int(got.sum())
    offset = torch.from_numpy((numpy.cumsum(got) - got).astype(numpy.int32)).to(dev)
    xy = torch.zeros((total, 4), dtype=torch.float64, device=dev)
    bary = torch.zeros((total, 2, 3), dtype=torch.float64, device=dev)
    level = torch.zeros(total, dtype=torch.int32, device=dev)
    cell = torch.zeros(total, dtype=torch.int32, device=dev)
    keys = torch.zeros((total, 4), dtype=torch.int32, device=dev)
    _hip.check(hip.flow_isoline_emit(
        m, s, fp, L, _hip.i32(count, nc), _hip.i32(offset, nc), total, _hip.f64(xy),
        _hip.i32(level), _hip.i32(cell), _hip.i32(keys), _hip.f64(bary), st))
    cell_h, level_h = host(cell), host(level)
    marked = numpy.isin(cell_h, broken)
    assert marked.sum() == 2 and (level_h[marked] == -1).all()
    assert (host(keys)[marked] == -1).all()
    assert numpy.isnan(host(xy)[marked]).all() and numpy.isnan(host(bary)[marked]).all()
    keep = ~numpy.isin(case.seg['cell'], broken)
    assert numpy.array_equal(cell_h[~marked], case.seg['cell'][keep])
    assert numpy.array_equal(host(keys)[~marked], case.seg['keys'][keep])
    assert numpy.abs(host(xy)[~marked] - case.seg['xy'][keep]).max() \
        <= TOL * iref.diameter(V.mesh())
    # the measures leave such a cell out and stay finite
    work, res = device.empty(2 * 5 * 2), device.empty(10)
    _hip.check(hip.flow_isoline_measure(m, s, fp, L, _hip.f64(work), _hip.f64(res), st))
    assert numpy.isfinite(host(res)).all()
