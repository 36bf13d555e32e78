# -*- coding: utf-8 -*-
'''
Contour lines without a GPU (flow_amd/fem/isolines.py): the numpy restatement
(tests/isolines_reference.py) on fields it must get exactly, the chaining of
segments into polylines, watertightness, the tie rule, the refusals (all
raised before the device is touched), the exports and the three symbols.

Position convergence, measured here with the restatement (the length of the
contour x^2 + y^2 = 0.36 of the P2 nodal values, a quarter circle of radius
0.6 round the corner (0, 0) of the unit square, against 0.3 pi; nested meshes
UnitSquareMesh(8, 8) and UnitSquareMesh(16, 16)):

    P2   1.428549e-03 -> 2.937330e-04   ratio 4.8634

The contour is that of the piecewise-linear interpolant on the sub-triangles,
so second order predicts 4; the test asks for the measured ratio less 25 %.
'''
import importlib
import os

import numpy
import pytest

from flow_amd import fem

import isolines_reference as iref

# (fem.isolines is the function; the module it hides)
fiso = importlib.import_module('flow_amd.fem.isolines')

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the measured ratio above, less 25 %
MARGIN = iref.QUARTER_CIRCLE_MARGIN
assert MARGIN == 0.75 * 4.8634

A, hole_mesh, nodal, clip_square = iref.A, iref.hole_mesh, iref.nodal, iref.clip_square


# -- 1. the restatement on fields it must get exactly --------------------------------
@pytest.mark.parametrize('deg', [1, 2])
def test_linear_field_is_contoured_exactly(deg):
    mesh = fem.UnitSquareMesh(5, 4, 'crossed')
    V = fem.FunctionSpace(mesh, 'CG', deg)
    f = nodal(V, lambda x, y: A[0] * x + A[1] * y)
    # (no level within rounding of a nodal value: a segment of length 1e-17
    # has no direction to check)
    levels = [-0.2531, 0.0123, 0.1017, 0.3313, 0.5509]
    s = iref.segments(V.layout, f, levels)
    assert len(s['cell']) > 0 and set(s['level']) == set(range(5))
    for end in (s['xy'][:, 0:2], s['xy'][:, 2:4]):
        err = numpy.abs(end @ A - numpy.array(levels)[s['level']]).max()
        print('P%d: |a.x - c| max %.2e' % (deg, err))
        assert err <= 1e-14
    want = [clip_square(A, c) for c in levels]
    got_len = iref.length(V.layout, f, levels)
    got_area = iref.area(V.layout, f, levels)
    for k in range(5):
        print('P%d c=%g: length %.15f (%.15f) area %.15f (%.15f)'
              % (deg, levels[k], got_len[k], want[k][0], got_area[k], want[k][1]))
        assert abs(got_len[k] - want[k][0]) <= 1e-13
        assert abs(got_area[k] - want[k][1]) <= 1e-13
    # the above side is on the left: a turned by +90 degrees points along
    d = s['xy'][:, 2:4] - s['xy'][:, 0:2]
    assert ((d @ numpy.array([-A[1], A[0]])) < 0.0).all()
    # everything, nothing
    assert abs(iref.area(V.layout, f, -1e300)[0] - mesh.cell_areas().sum()) <= 1e-13
    assert iref.area(V.layout, f, 1e300)[0] == 0.0
    for c in (-0.5, 0.8):            # outside [-0.4, 0.7]
        assert len(iref.segments(V.layout, f, c)['cell']) == 0
        assert iref.length(V.layout, f, c)[0] == 0.0
    const = numpy.full(V.N, 0.25)
    assert len(iref.segments(V.layout, const, 0.25)['cell']) == 0
    assert iref.length(V.layout, const, 0.25)[0] == 0.0
    assert abs(iref.area(V.layout, const, 0.25)[0] - 1.0) <= 1e-13


# -- 2. chaining ---------------------------------------------------------------------
def _keys(pairs):
    '''Segments from a list of (start key, end key).'''
    return numpy.array([s + e for s, e in pairs], dtype=numpy.int32)


def test_chain_an_open_line_and_a_closed_loop():
    e = [(0, 1), (1, 2), (2, 3), (3, 4)]                 # an open line, in order
    q = [(10, 11), (11, 12), (12, 13)]                   # a loop
    keys = _keys([(e[1], e[2]), (q[0], q[1]), (e[0], e[1]), (q[2], q[0]),
                  (e[2], e[3]), (q[1], q[2])])
    (lines,) = fiso.chain_segments(keys, numpy.zeros(6, dtype=int), 1)
    assert [(idx.tolist(), closed) for idx, closed in lines] == [
        ([2, 0, 4], False), ([1, 5, 3], True)]


def test_chain_two_levels_interleaved():
    a = [(0, 1), (1, 2), (2, 3)]
    b = [(5, 6), (6, 7), (7, 8)]
    keys = _keys([(a[0], a[1]), (b[1], b[2]), (a[1], a[2]), (b[0], b[1])])
    level = numpy.array([0, 1, 0, 1])
    lines = fiso.chain_segments(keys, level, 3)
    assert len(lines) == 3 and lines[2] == []
    assert [(i.tolist(), c) for i, c in lines[0]] == [([0, 2], False)]
    assert [(i.tolist(), c) for i, c in lines[1]] == [([3, 1], False)]
    # the same keys on two levels do not join across them
    both = fiso.chain_segments(_keys([(a[0], a[1]), (a[1], a[2])]), [0, 1], 2)
    assert [[(i.tolist(), c) for i, c in per] for per in both] == [
        [([0], False)], [([1], False)]]


def test_chain_a_shuffled_loop_starts_at_its_smallest_key():
    ring = [(7, 9), (3, 4), (3, 8), (2, 30), (5, 6)]
    segs = [(ring[i], ring[(i + 1) % 5]) for i in range(5)]
    perm = [3, 0, 4, 2, 1]
    keys = _keys([segs[i] for i in perm])
    (lines,) = fiso.chain_segments(keys, numpy.zeros(5, dtype=int), 1)
    assert len(lines) == 1 and lines[0][1] is True
    walked = [perm[i] for i in lines[0][0]]
    assert walked == [3, 4, 0, 1, 2]                     # from key (2, 30) on
    assert fiso.chain_segments(numpy.zeros((0, 4)), [], 2) == [[], []]


# -- 3. watertight -------------------------------------------------------------------
@pytest.mark.parametrize('deg', [1, 2])
def test_watertight_on_the_hole_mesh(deg):
    mesh = hole_mesh()
    assert mesh.num_cells() < 2 * 9 * 7               # the hole is there
    V = fem.FunctionSpace(mesh, 'CG', deg)
    f = nodal(V, lambda x, y: numpy.sin(3 * x) * numpy.cos(2 * y))
    levels = numpy.linspace(f.min(), f.max(), 7)[1:-1]
    tri = iref.Triangulation(V.layout)
    s = iref.segments(V.layout, f, levels, tri)
    boundary = tri.boundary_keys()
    closed_or_to_the_wall = 0
    for k in range(5):
        sel = s['level'] == k
        assert sel.sum() > 0
        starts = list(map(tuple, s['keys'][sel, 0:2].tolist()))
        ends = list(map(tuple, s['keys'][sel, 2:4].tolist()))
        assert len(set(starts)) == len(starts) and len(set(ends)) == len(ends)
        for key in set(starts) | set(ends):
            assert key[0] < key[1]
            if key in boundary:
                assert (key in starts) != (key in ends), key
            else:
                assert key in starts and key in ends, key
        # ... so every chained line is closed or runs from wall to wall
        (lines,) = fiso.chain_segments(s['keys'][sel], numpy.zeros(sel.sum(), int), 1)
        for idx, closed in lines:
            keys = s['keys'][sel][idx]
            assert (keys[1:, 0:2] == keys[:-1, 2:4]).all()
            if closed:
                assert tuple(keys[-1, 2:4]) == tuple(keys[0, 0:2])
            else:
                assert tuple(keys[0, 0:2]) in boundary
                assert tuple(keys[-1, 2:4]) in boundary
            closed_or_to_the_wall += 1
    assert closed_or_to_the_wall >= 5


# -- 4. the tie rule -----------------------------------------------------------------
@pytest.mark.parametrize('deg', [1, 2])
def test_nodes_on_the_level_give_no_empty_and_no_double_segment(deg):
    mesh = fem.UnitSquareMesh(5, 4, 'crossed')
    V = fem.FunctionSpace(mesh, 'CG', deg)
    f = nodal(V, lambda x, y: numpy.round(4 * x) + numpy.round(4 * y))
    levels = numpy.arange(0.0, 10.0)                  # the range is [0, 8]
    assert (f == numpy.round(f)).all() and f.min() == 0.0 and f.max() == 8.0
    s = iref.segments(V.layout, f, levels)
    assert len(s['cell']) > 0
    seg_len = numpy.hypot(s['xy'][:, 2] - s['xy'][:, 0], s['xy'][:, 3] - s['xy'][:, 1])
    print('P%d: %d segments, shortest %.3e' % (deg, len(seg_len), seg_len.min()))
    assert seg_len.min() > 1e-3
    rows = numpy.column_stack([s['level'], s['keys']])
    assert len(numpy.unique(rows, axis=0)) == len(rows)
    # ... nor the same segment walked the other way
    back = numpy.column_stack([s['level'], s['keys'][:, 2:4], s['keys'][:, 0:2]])
    assert len(numpy.unique(numpy.concatenate([rows, back]), axis=0)) == 2 * len(rows)
    # nodes lie on the levels, and nothing is lost by the rule: level 0 is
    # the whole mesh, level 9 nothing
    assert (s['level'] >= 1).all() and (s['level'] <= 8).all()
    area = iref.area(V.layout, f, levels)
    assert abs(area[0] - 1.0) <= 1e-13 and area[9] == 0.0
    assert (numpy.diff(area) <= 0.0).all()


# -- 5. refusals, exports, symbols ---------------------------------------------------
def test_refusals(monkeypatch):
    mesh = fem.UnitSquareMesh(4, 4)
    other = fem.UnitSquareMesh(4, 4)
    P1, P2 = fem.FunctionSpace(mesh, 'CG', 1), fem.FunctionSpace(mesh, 'CG', 2)
    W = fem.VectorFunctionSpace(mesh, 'CG', 2)
    mixed = fem.FunctionSpace(
        mesh, fem.VectorElement('CG', 'triangle', 2)
        * fem.FiniteElement('CG', 'triangle', 1))
    for V in (mixed, W, W.sub(0), W.sub(1)):
        with pytest.raises(NotImplementedError):
            fem.Isolines(V)
    with pytest.raises(NotImplementedError):
        fem.isolines(fem.Function(W), 0.0)
    with pytest.raises(ValueError, match='f:'):
        fem.isolines(3.0, 0.0)

    class Cubic(object):
        layout, component, degree, dim = P2.layout, None, 3, 1

    with pytest.raises(NotImplementedError, match='P3'):
        fem.Isolines(Cubic())
    I = fem.Isolines(P2)
    f = fem.Function(P2)
    for bad in (fem.Function(P1), fem.Function(W),
                fem.Function(fem.FunctionSpace(other, 'CG', 2)), 3.0):
        for call in (I.extract, I.length, I.area):
            with pytest.raises(ValueError, match='f:'):
                call(bad, 0.0)
    for bad in ([], numpy.zeros(0), [0.0, numpy.nan], numpy.inf, -numpy.inf,
                [[0.0, 1.0]], 'high', None):
        for call in (I.extract, I.length, I.area):
            with pytest.raises(ValueError, match='levels'):
                call(f, bad)
        with pytest.raises(ValueError, match='levels'):
            fem.isolines(f, bad)
    empty = fiso.Contours(P2, numpy.array([0.0]), 0, None, None, None, None, None)
    for t in (-1e-3, 1.001, numpy.nan, numpy.inf):
        with pytest.raises(ValueError, match='t:'):
            empty.evaluate(f, t=t)
    assert empty.polylines() == [[]] and empty.polylines(0) == []
    with pytest.raises(ValueError, match='k:'):
        empty.polylines(1)
    from flow_amd import parallel
    monkeypatch.setattr(parallel, 'active', lambda: True)
    for call in (lambda: fem.Isolines(P2), lambda: I.extract(f, 0.0),
                 lambda: I.length(f, 0.0), lambda: I.area(f, [0.0, 1.0]),
                 lambda: fem.isolines(f, 0.0), lambda: empty.evaluate(f)):
        with pytest.raises(NotImplementedError, match='on strips'):
            call()


def test_exports():
    for name in ('Isolines', 'isolines'):
        assert getattr(fem, name) is getattr(fiso, name)
    assert callable(fiso.chain_segments)


def test_symbols_declared_and_bound():
    import ctypes
    from flow_amd import _hip
    with open(os.path.join(ROOT, 'include', 'flow_hip.h')) as f:
        header = f.read()
    lib = _hip.load_library()
    assert lib.flow_abi_version() == 30 == _hip.ABI_VERSION
    for name, nargs in (('flow_isoline_count', 6), ('flow_isoline_emit', 13),
                        ('flow_isoline_measure', 7)):
        assert 'int %s(' % name in header
        assert len(_hip.SYMBOLS[name]) == nargs
        decl = header[header.index('int %s(' % name):]
        assert decl[:decl.index(';')].count(',') == nargs - 1
        assert getattr(lib, name) is not None
    assert '#define FLOW_ISOLINE_LEVELS_PER_LAUNCH %d' \
        % _hip.ISOLINE_LEVELS_PER_LAUNCH in header
    assert _hip.ISOLINE_LEVELS_PER_LAUNCH == 32
    assert ctypes.sizeof(_hip.IsolineLevels) == 8 + 8 * 32
    with open(os.path.join(ROOT, 'flow_amd', 'csrc', 'Makefile')) as f:
        assert 'isoline_kernels.hip' in f.read()


def test_entry_points_check_their_arguments_before_anything_else():
    '''Refused calls return FLOW_INVALID without a device: the addresses
    below are never read.'''
    import ctypes
    from flow_amd import _hip
    lib = _hip.load_library()
    p, q = ctypes.c_void_p(4096), ctypes.c_void_p(8192)
    mesh = _hip.MeshS(10, p)
    space = _hip.SpaceS(2, 30, 100, p, p, p, p, p)
    lev = _hip.IsolineLevels(1, 0)
    count = _hip.launch_count()

    def variant(cls, base, **fields):
        s = cls.from_buffer_copy(base)
        for key, value in fields.items():
            setattr(s, key, value)
        return s

    def ref(s):
        return ctypes.byref(s) if s is not None else None

    def calls(m, s, f=p, L=lev, count=True):
        return ([
            lib.flow_isoline_count(ref(m), ref(s), f, ref(L), p, None)]
            if count else []) + [
            lib.flow_isoline_emit(ref(m), ref(s), f, ref(L), p, p, 8, p, p, p, p,
                                  p, None),
            lib.flow_isoline_measure(ref(m), ref(s), f, ref(L), p, q, None)]

    refused = []
    for m, s, f, L in [
            (None, space, p, lev), (mesh, None, p, lev), (mesh, space, None, lev),
            (mesh, space, p, None),
            (variant(_hip.MeshS, mesh, nc=0), space, p, lev),
            (variant(_hip.MeshS, mesh, c1=1), space, p, lev),
            (mesh, variant(_hip.SpaceS, space, deg=3), p, lev),
            (mesh, variant(_hip.SpaceS, space, deg=0), p, lev),
            (mesh, variant(_hip.SpaceS, space, n=0), p, lev),
            (mesh, variant(_hip.SpaceS, space, cell_dofs=None), p, lev),
            (mesh, variant(_hip.SpaceS, space, r1=1), p, lev),
            (mesh, space, p, _hip.IsolineLevels(33, 0)),
            (mesh, space, p, _hip.IsolineLevels(-1, 0)),
            (mesh, space, p, _hip.IsolineLevels(1, -1))]:
        refused += calls(m, s, f, L)
    no_xy = variant(_hip.MeshS, mesh, xy=None)
    refused += calls(no_xy, space, count=False)       # the count reads no xy
    refused += [
        lib.flow_isoline_count(ref(mesh), ref(space), p, ref(lev), None, None),
        lib.flow_isoline_emit(ref(mesh), ref(space), p, ref(lev), None, p, 8, p, p,
                              p, p, p, None),
        lib.flow_isoline_emit(ref(mesh), ref(space), p, ref(lev), p, None, 8, p, p,
                              p, p, p, None),
        lib.flow_isoline_emit(ref(mesh), ref(space), p, ref(lev), p, p, -1, p, p,
                              p, p, p, None),
        lib.flow_isoline_measure(ref(mesh), ref(space), p, ref(lev), None, q, None),
        lib.flow_isoline_measure(ref(mesh), ref(space), p, ref(lev), p, None, None),
        lib.flow_isoline_measure(ref(mesh), ref(space), p, ref(lev), p, p, None)]
    for k in range(7, 12):                            # each output of the emit
        args = [ref(mesh), ref(space), p, ref(lev), p, p, 8, p, p, p, p, p, None]
        args[k] = None
        refused.append(lib.flow_isoline_emit(*args))
    assert refused == [2] * len(refused)
    with pytest.raises(ValueError, match='invalid argument'):
        _hip.check(2)
    # no level, no capacity: nothing to do
    none = _hip.IsolineLevels(0, 0)
    assert calls(mesh, space, L=none) == [0, 0, 0]
    assert lib.flow_isoline_emit(ref(mesh), ref(space), p, ref(lev), p, p, 0, None,
                                 None, None, None, None, None) == 0
    assert _hip.launch_count() == count


# -- 6. position convergence ---------------------------------------------------------
quarter_circle_errors = iref.quarter_circle_errors


def test_position_converges_on_the_quarter_circle():
    errs = quarter_circle_errors(
        lambda V, f, c: iref.length(V.layout, f, c)[0])
    print('P2: %.6e -> %.6e, ratio %.4f (asked: %.4f)'
          % (errs[0], errs[1], errs[0] / errs[1], MARGIN))
    assert errs[1] < errs[0] / MARGIN
