# -*- coding: utf-8 -*-
'''
Connected components of level sets on the HIP path (flow_amd/fem/regions.py;
csrc/region_kernels.hip) against the numpy / scipy restatement of tests/
regions_reference.py.

Meshes: UnitSquareMesh(5, 4, 'crossed') (less than one block),
UnitSquareMesh(12, 11) (264 cells: the last block is partial; on P2 1056
slots, more than a block strides over at once) and the small
rectangle_with_hole of the host tests; P1 and P2 on each.  The field is
sin(3 pi x + 0.4) cos(2 pi y - 0.3) as nodal values, {f >= 0.25} and
{f < -0.25}.

Labels, roots, sizes, counts and extrema are integers or copies: exact.  The
integrals are sums of at most 8 nc triangle integrals added in another order
than the restatement's (and with g interpolated along the sub-edges instead of
evaluated at the physical point): 1e-12 * the sum of the |triangle integrals|
of that component and row, Isolines' bound.

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

import regions_reference as rref
from regions_reference import Triangulation, hole_mesh, nodal

freg = importlib.import_module('flow_amd.fem.regions')

pytestmark = pytest.mark.gpu

TOL = 1e-12
MESHES = ('crossed 5x4', 'square 12x11', 'hole')
SIDES = (('above', 0.25), ('below', -0.25))
EVERY = freg.CHECK_EVERY


@functools.lru_cache(maxsize=None)
def _mesh(name):
    if name == 'hole':
        return hole_mesh()
    if name == 'crossed 5x4':
        return fem.UnitSquareMesh(5, 4, 'crossed')
    if name == 'one':
        return fem.UnitSquareMesh(1, 1)
    return fem.UnitSquareMesh(12, 11)


@functools.lru_cache(maxsize=None)
def _space(name, deg, dim=1):
    if dim == 1:
        return fem.FunctionSpace(_mesh(name), 'CG', deg)
    return fem.VectorFunctionSpace(_mesh(name), 'CG', deg)


@functools.lru_cache(maxsize=None)
def _tri(name, deg):
    return Triangulation(_space(name, deg).layout)


def _wave(x, y):
    return numpy.sin(3 * numpy.pi * x + 0.4) * numpy.cos(2 * numpy.pi * y - 0.3)


def _g_values(W):
    '''Nodal values (dim, N) of a smooth field that is no polynomial.'''
    xy = W.layout.dof_coords
    rows = [numpy.exp(xy[:, 0]) * numpy.cos(3 * xy[:, 1]) - 0.3,
            numpy.sin(2 * xy[:, 0] - xy[:, 1])]
    return numpy.array(rows[:W.dim])


def function(V, values):
    f = fem.Function(V)
    f.set_array(numpy.ascontiguousarray(values, dtype=float).reshape(-1))
    return f


def host(t):
    return device.to_host(t).numpy()


def reference(name, deg, values, level, side, W=None):
    V = _space(name, deg)
    g = None if W is None else _g_values(W)
    r = rref.regions(V.layout, values, level, side=side, g=g,
                     glayout=None if W is None else W.layout, tri=_tri(name, deg))
    for a in r.values():
        if isinstance(a, numpy.ndarray):
            a.flags.writeable = False
    return r


@functools.lru_cache(maxsize=None)
def _wave_case(name, deg, side, level, gdeg=None, gdim=1):
    V = _space(name, deg)
    W = None if gdeg is None else _space(name, gdeg, gdim)
    return reference(name, deg, nodal(V, _wave), level, side, W)


def check_labels(C, want):
    assert C.count == want['count']
    assert numpy.array_equal(host(C.labels), want['labels'])
    assert numpy.array_equal(host(C.root), want['root'])
    assert numpy.array_equal(host(C.size), want['size'])
    assert C.labels.dtype == C.root.dtype == C.size.dtype == torch.int32
    assert tuple(C.labels.shape) == (C.V.N,)
    assert tuple(C.root.shape) == tuple(C.size.shape) == (C.count,)
    assert C.sweeps > 0 and C.sweeps % EVERY == 0


def check_measures(C, want, what):
    '''area and centroid * area against the restatement; the largest error
    in units of the bound.'''
    assert C.area.dtype == C.centroid.dtype == torch.float64
    assert tuple(C.area.shape) == (C.count,) and tuple(C.centroid.shape) == (C.count, 2)
    area, centroid = host(C.area), host(C.centroid)
    # a component all of whose sub-triangles hold a non-finite value has no
    # piece: its area is 0 and its centroid, 0 / 0, is NaN
    bare = want['scale'][0] == 0.0
    assert (area[bare] == 0.0).all() and numpy.isnan(centroid[bare]).all()
    keep = ~bare
    got = numpy.vstack([area, (centroid * area[:, None]).T])[:, keep]
    worst = 0.0
    if keep.any():
        err = numpy.abs(got - want['moments'][:3, keep])
        bound = TOL * want['scale'][:3, keep]
        worst = (err / bound).max()
        print('%s: area, centroid * area: %.2e of the bound' % (what, worst))
        assert (bound > 0.0).all() and (err <= bound).all()
    return worst


# -- 1. labels -----------------------------------------------------------------------
@pytest.mark.parametrize('side,level', SIDES)
@pytest.mark.parametrize('deg', [1, 2])
@pytest.mark.parametrize('name', MESHES)
def test_labels_against_reference(hip, name, deg, side, level):
    V = _space(name, deg)
    want = _wave_case(name, deg, side, level)
    # what the case claims: three components or more, one at the boundary
    assert want['count'] >= 3
    on_boundary = numpy.zeros(V.N, dtype=bool)
    on_boundary[numpy.array(sorted(_tri(name, deg).boundary_keys())).ravel()] = True
    touching = numpy.unique(want['labels'][on_boundary & (want['labels'] >= 0)])
    assert len(touching) >= 1
    f = function(V, nodal(V, _wave))
    C = fem.Regions(V).label(f, level, side=side)
    print('%s P%d %s: %d components (%d at the boundary), sizes %s, %d sweeps'
          % (name, deg, side, C.count, len(touching), want['size'].tolist(), C.sweeps))
    check_labels(C, want)
    check_measures(C, want, '%s P%d %s' % (name, deg, side))
    # the one-off spelling
    D = fem.regions(f, level, side=side)
    assert torch.equal(D.labels, C.labels) and torch.equal(D.area, C.area)


# -- 2. batching ---------------------------------------------------------------------
def _serpentine(V):
    '''0 / 1 nodal values on UnitSquareMesh(12, 11): every second grid row,
    joined at alternating ends (in half steps of the grid, so that P2's mid
    points follow the same rule).'''
    xy = V.layout.dof_coords
    i = numpy.round(xy[:, 0] * 24).astype(int)
    j = numpy.round(xy[:, 1] * 22).astype(int)
    ins = (j % 4 == 0) | ((i == 24) & numpy.isin(j % 8, (1, 2, 3))) \
        | ((i == 0) & numpy.isin(j % 8, (5, 6, 7)))
    return ins.astype(float)


@pytest.mark.parametrize('deg', [1, 2])
def test_batches_and_the_pointer_jump(hip, deg):
    name = 'square 12x11'
    V = _space(name, deg)
    values = _serpentine(V)
    want = reference(name, deg, values, 0.5, 'above')
    diameter = rref.diameter(_tri(name, deg), values >= 0.5)
    # the plain neighbour minimum moves one sub-edge per sweep
    assert want['count'] == 1 and diameter > 2 * EVERY
    R = fem.Regions(V)
    C = R.label(function(V, values), 0.5)
    print('P%d: diameter %d sub-edges, %d sweeps in batches of %d'
          % (deg, diameter, C.sweeps, EVERY))
    check_labels(C, want)
    assert C.sweeps < diameter
    # one further batch on the fixed point: unchanged, the flag stays 0
    raw = torch.where(C.labels >= 0, C.root[C.labels.clamp(min=0).long()],
                      torch.full_like(C.labels, -1)).contiguous()
    a, b = raw.clone(), torch.full_like(raw, -7)
    flag = torch.zeros(1, dtype=torch.int32, device=device.get())
    launches = _hip.launch_count()
    _hip.check(hip.flow_region_sweeps(
        ctypes.byref(ops.mesh_struct(V.mesh())), ctypes.byref(ops.space_struct(V.layout)),
        EVERY, _hip.i32(a, V.N), _hip.i32(b, V.N), _hip.i32(flag, 1), _hip.stream()))
    assert _hip.launch_count() == launches + EVERY
    assert int(host(flag)[0]) == 0
    assert torch.equal(a, raw) and torch.equal(b, raw)


# -- 3. measures ---------------------------------------------------------------------
@pytest.mark.parametrize('deg,gdeg,gdim', [(1, 1, 1), (1, 2, 1), (2, 1, 1), (2, 2, 1),
                                           (1, 2, 2), (2, 2, 2), (2, 1, 2)])
@pytest.mark.parametrize('name', MESHES)
def test_integrals_and_extrema_against_reference(hip, name, deg, gdeg, gdim):
    V, W = _space(name, deg), _space(name, gdeg, gdim)
    side, level = SIDES[0]
    want = _wave_case(name, deg, side, level, gdeg, gdim)
    C = fem.Regions(V).label(function(V, nodal(V, _wave)), level, side=side)
    check_labels(C, want)
    check_measures(C, want, '%s P%d' % (name, deg))
    g = function(W, _g_values(W))
    got = host(C.integrate(g))
    assert got.shape == (gdim, C.count) and got.dtype == numpy.float64
    err = numpy.abs(got - want['moments'][3:])
    bound = TOL * want['scale'][3:]
    print('%s P%d, g P%d^%d: integrals %.2e of the bound'
          % (name, deg, gdeg, gdim, (err / bound).max()))
    assert (bound > 0.0).all() and (err <= bound).all()
    if gdeg == deg:
        lo, hi = C.extrema(g)
        assert lo.dtype == hi.dtype == torch.float64
        assert numpy.array_equal(host(lo), want['gmin'])
        assert numpy.array_equal(host(hi), want['gmax'])
    else:
        with pytest.raises(ValueError, match='dofs of V'):
            C.extrema(g)


# -- 4. cross-checks -----------------------------------------------------------------
@pytest.mark.parametrize('deg', [1, 2])
@pytest.mark.parametrize('name', MESHES)
def test_areas_against_isolines_and_the_mesh(hip, name, deg):
    V = _space(name, deg)
    f = function(V, nodal(V, _wave))
    R = fem.Regions(V)
    up, down = R.label(f, 0.25), R.label(f, 0.25, side='below')
    above = float(host(up.area.sum()))
    iso = fem.Isolines(V).area(f, 0.25)[0]
    total = V.mesh().cell_areas().sum()
    both = above + float(host(down.area.sum()))
    print('%s P%d: areas %.15f, Isolines %.15f (%.2e); above + below %.15f, mesh '
          '%.15f (%.2e)' % (name, deg, above, iso, abs(above / iso - 1.0), both, total,
                            abs(both / total - 1.0)))
    assert abs(above / iso - 1.0) <= TOL
    assert abs(both / total - 1.0) <= TOL
    assert ((host(up.labels) >= 0) != (host(down.labels) >= 0)).all()


def _triangle_area(a, b, c):
    '''add_triangle's formula (csrc/region_kernels.hip), in fp64.'''
    return 0.5 * abs((b[0] - a[0]) * (c[1] - a[1]) - (c[0] - a[0]) * (b[1] - a[1]))


@pytest.mark.parametrize('deg', [1, 2])
@pytest.mark.parametrize('name', ['one', 'crossed 5x4'])
def test_pieces_end_on_the_crossings_of_isolines(hip, name, deg):
    '''Regions cuts a sub-triangle at the crossings Isolines emits (one
    `cross` in csrc/subtri.h): the area of every cut piece, rebuilt on the
    host from the end points of that sub-triangle's segment in Contours.xy
    and the positions of its inside nodes, is the slot's area of the moments
    launch.  Both sides evaluate add_triangle's expression on the same bits;
    the kernel may contract its two products into one fma and the host does
    not, a difference of at most 2^-53 (|u_x v_y| + |v_x u_y|) per triangle:
    1e-14 relative leaves a factor of 90 for the pieces' shape.'''
    from isolines_reference import SUBS
    V, level = _space(name, deg), 0.25
    mesh, cell_dofs = V.mesh(), numpy.asarray(V.layout.cell_dofs)
    nc = mesh.num_cells()
    values = nodal(V, _wave)
    f = function(V, values)
    R = fem.Regions(V)
    assert R.label(f, level).count >= 1
    keys = host(R._buffers()[3]).reshape(-1, nc)
    areas = host(R._buffers()[4][0]).reshape(-1, nc)
    S = fem.Isolines(V).extract(f, level)
    xy, cell, skeys = host(S.xy), host(S.cell), host(S.keys)
    seen, worst = {1: 0, 2: 0}, 0.0
    for k in range(S.nseg):
        c, dofs = cell[k], cell_dofs[cell[k]]
        v = mesh.points[mesh.cell_vertices[c]]
        X = [v[0], v[1], v[2], 0.5 * (v[1] + v[2]), 0.5 * (v[0] + v[2]),
             0.5 * (v[0] + v[1])]
        (s,) = [s for s, sub in enumerate(SUBS[deg])
                if set(dofs[list(sub)]) == set(skeys[k])]
        sub = SUBS[deg][s]
        assert keys[s, c] >= 0                 # Regions holds a piece of it
        # P, alone on its side: the dof on both crossed sub-edges; Q and R
        # behind it in the cell's cyclic order
        (lone,) = set(skeys[k, :2]) & set(skeys[k, 2:])
        p = [dofs[m] for m in sub].index(lone)
        P, Q, Rn = sub[p], sub[(p + 1) % 3], sub[(p + 2) % 3]
        ends = {frozenset(skeys[k, :2].tolist()): xy[k, :2],
                frozenset(skeys[k, 2:].tolist()): xy[k, 2:]}
        pq = ends[frozenset((dofs[P], dofs[Q]))]
        pr = ends[frozenset((dofs[P], dofs[Rn]))]
        nin = int((values[dofs[list(sub)]] >= level).sum())
        if nin == 1:
            assert values[lone] >= level
            want = _triangle_area(X[P], pq, pr)
        else:
            assert nin == 2 and values[lone] < level
            want = _triangle_area(X[Q], X[Rn], pr) + _triangle_area(X[Q], pr, pq)
        seen[nin] += 1
        assert want > 0.0
        worst = max(worst, abs(areas[s, c] - want) / want)
    print('%s P%d: %d pieces with one inside node, %d with two: areas differ by '
          '%.2e relative at most' % (name, deg, seen[1], seen[2], worst))
    # what the case claims: one node alone above in some sub-triangle, two in another
    assert seen[1] >= 1 and seen[2] >= 1
    assert worst <= 1e-14


# -- 5. a P2 cell split between two components -----------------------------------------
def test_two_components_in_one_p2_cell(hip):
    V = _space('one', 2)
    values = numpy.zeros(V.N)
    corners = V.layout.vertex_dofs[V.mesh().cell_vertices[0, :2]]
    values[corners] = 1.0
    want = reference('one', 2, values, 0.5, 'above')
    # two vertices of cell 0 inside, every mid point outside
    assert want['count'] == 2 and want['size'].tolist() == [1, 1]
    assert (values[V.layout.edge_dofs] == 0.0).all()
    R = fem.Regions(V)
    C = R.label(function(V, values), 0.5)
    check_labels(C, want)
    check_measures(C, want, 'one cell P2')
    assert sorted(host(C.root).tolist()) == sorted(corners.tolist())
    # ... two pieces with different keys in the slots of cell 0
    keys = host(R._buffers()[3]).reshape(4, V.mesh().num_cells())
    assert sorted(k for k in keys[:, 0].tolist() if k >= 0) == [0, 1]


# -- 6. non-finite values ------------------------------------------------------------
@pytest.mark.parametrize('side,level', SIDES)
@pytest.mark.parametrize('deg', [1, 2])
def test_non_finite_values_are_outside(hip, deg, side, level):
    name = 'square 12x11'
    V = _space(name, deg)
    values = nodal(V, _wave).copy()
    bad = numpy.arange(7, V.N, 23)
    values[bad] = numpy.inf
    values[bad[1]] = -numpy.inf
    values[bad[3]] = numpy.nan
    clean = _wave_case(name, deg, side, level)
    want = reference(name, deg, values, level, side)
    assert want['area'].sum() < clean['area'].sum()
    W = _space(name, 2)
    wantg = reference(name, deg, values, level, side, W)
    C = fem.Regions(V).label(function(V, values), level, side=side)
    check_labels(C, want)
    assert (host(C.labels)[bad] == -1).all()
    check_measures(C, want, 'P%d %s' % (deg, side))
    got = host(C.integrate(function(W, _g_values(W))))
    assert numpy.isfinite(got).all()
    assert (numpy.abs(got - wantg['moments'][3:]) <= TOL * wantg['scale'][3:]).all()


# -- 7. edges ------------------------------------------------------------------------
@pytest.mark.parametrize('deg', [1, 2])
def test_nothing_everything_and_a_field_on_the_level(hip, deg):
    name = 'square 12x11'
    V = _space(name, deg)
    R = fem.Regions(V)
    const = function(V, numpy.full(V.N, 0.25))
    g = function(_space(name, 2, 2), _g_values(_space(name, 2, 2)))
    own = function(V, _g_values(V))
    R.label(const, 0.0)                                   # the buffers exist
    for f, level, side in ((const, 0.26, 'above'), (const, 0.25, 'below'),
                           (const, 0.0, 'below')):
        launches = _hip.launch_count()
        C = R.label(f, level, side=side)
        # the initialisation and one batch: no moments, no segment launch
        assert _hip.launch_count() == launches + 1 + EVERY
        assert C.count == 0 and C.sweeps == EVERY
        assert (host(C.labels) == -1).all() and C.labels.dtype == torch.int32
        for t, shape, dtype in ((C.root, (0,), torch.int32), (C.size, (0,), torch.int32),
                                (C.area, (0,), torch.float64),
                                (C.centroid, (0, 2), torch.float64),
                                (C.integrate(g), (2, 0), torch.float64),
                                (C.extrema(own)[0], (1, 0), torch.float64),
                                (C.extrema(own)[1], (1, 0), torch.float64)):
            assert tuple(t.shape) == shape and t.dtype == dtype and t.is_cuda
        assert _hip.launch_count() == launches + 1 + EVERY
        assert (C.as_function().array() == -1.0).all()
        with pytest.raises(ValueError, match='k:'):
            C.mask(0)
    total = V.mesh().cell_areas().sum()
    for f, level, side in ((const, 0.25, 'above'), (const, 0.0, 'above'),
                           (const, 0.26, 'below')):
        C = R.label(f, level, side=side)
        assert C.count == 1 and host(C.root).tolist() == [0]
        assert host(C.size).tolist() == [V.N] and (host(C.labels) == 0).all()
        assert abs(float(host(C.area)[0]) / total - 1.0) <= TOL
        assert numpy.abs(host(C.centroid)[0] - 0.5).max() <= TOL


# -- 8. the same bits ----------------------------------------------------------------
@pytest.mark.parametrize('deg', [1, 2])
@pytest.mark.parametrize('name', ['square 12x11', 'hole'])
def test_same_bits_twice(hip, name, deg):
    V, W = _space(name, deg), _space(name, 2, 2)
    f, g = function(V, nodal(V, _wave)), function(W, _g_values(W))
    own = function(V, _g_values(V))
    outs = []
    for R in (fem.Regions(V), fem.Regions(V)):
        C = R.label(f, 0.25)
        lo, hi = C.extrema(own)
        outs.append((C.labels, C.root, C.size, C.area, C.centroid, C.integrate(g),
                     lo, hi))
    assert outs[0][0].data_ptr() != outs[1][0].data_ptr()
    for a, b in zip(*outs):
        assert numpy.array_equal(host(a), host(b))
    # ... and from one Regions used twice
    C = R.label(f, 0.25)
    assert torch.equal(C.area, outs[0][3]) and torch.equal(C.integrate(g), outs[0][5])


# -- 9. the indicator as a form operand ------------------------------------------------
@pytest.mark.parametrize('deg', [1, 2])
def test_as_function_and_mask(hip, deg):
    name = 'square 12x11'
    V = _space(name, deg)
    total = V.mesh().cell_areas().sum()
    C = fem.Regions(V).label(function(V, numpy.ones(V.N)), 0.5)
    assert C.count == 1
    ind = C.as_function()
    assert ind.function_space() is V
    dx = fem.dx(V.mesh(), degree=2)
    got = fem.assemble(fem.conditional(fem.eq(ind, 0.0), 1.0, 0.0) * dx)
    miss = fem.assemble(fem.conditional(fem.eq(ind, 1.0), 1.0, 0.0) * dx)
    print('P%d: the indicator integrates to %.15f, the mesh has %.15f' % (deg, got, total))
    assert abs(got / total - 1.0) <= TOL and miss == 0.0
    D = fem.Regions(V).label(function(V, nodal(V, _wave)), 0.25)
    labels = host(D.labels)
    assert numpy.array_equal(D.as_function().array(), labels.astype(float))
    for k in range(D.count):
        m = D.mask(k)
        assert m.function_space() is V
        assert numpy.array_equal(m.array(), (labels == k).astype(float))
    for k in (-1, D.count):
        with pytest.raises(ValueError, match='k:'):
            D.mask(k)


# -- 10. the entry points refuse what they cannot run --------------------------------
def test_argument_errors_launch_nothing(hip):
    V = _space('square 12x11', 2)
    N, nc = V.N, V.mesh().num_cells()
    mesh_s, space_s = ops.mesh_struct(V.mesh()), ops.space_struct(V.layout)
    m, s = ctypes.byref(mesh_s), ctypes.byref(space_s)
    f = function(V, nodal(V, _wave))
    dev = device.get()
    fp = _hip.f64(f.data, N)
    a = torch.zeros(N, dtype=torch.int32, device=dev)
    b = torch.zeros(N, dtype=torch.int32, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    keys = torch.zeros(4 * nc, dtype=torch.int32, device=dev)
    vals = device.empty(5 * 4 * nc)
    out = device.empty(16)
    pa, pb, pf = _hip.i32(a, N), _hip.i32(b, N), _hip.i32(flag, 1)
    pk, pv, po = _hip.i32(keys), _hip.f64(vals), _hip.f64(out)
    st = _hip.stream()
    strips = _hip.MeshS.from_buffer_copy(mesh_s)
    strips.c1 = 1
    cubic = _hip.SpaceS.from_buffer_copy(space_s)
    cubic.deg = 3
    launches = _hip.launch_count()
    refused = [
        hip.flow_region_init(None, fp, 0.25, 0, pa, st),
        hip.flow_region_init(s, None, 0.25, 0, pa, st),
        hip.flow_region_init(s, fp, 0.25, 0, None, st),
        hip.flow_region_init(s, fp, float('nan'), 0, pa, st),
        hip.flow_region_init(s, fp, 0.25, 2, pa, st),
        hip.flow_region_sweeps(None, s, EVERY, pa, pb, pf, st),
        hip.flow_region_sweeps(m, None, EVERY, pa, pb, pf, st),
        hip.flow_region_sweeps(ctypes.byref(strips), s, EVERY, pa, pb, pf, st),
        hip.flow_region_sweeps(m, ctypes.byref(cubic), EVERY, pa, pb, pf, st),
        hip.flow_region_sweeps(m, s, 0, pa, pb, pf, st),
        hip.flow_region_sweeps(m, s, EVERY, None, pb, pf, st),
        hip.flow_region_sweeps(m, s, EVERY, pa, None, pf, st),
        hip.flow_region_sweeps(m, s, EVERY, pa, pb, None, st),
        hip.flow_region_sweeps(m, s, EVERY, pa, pa, pf, st),
        hip.flow_region_moments(None, s, fp, 0.25, pa, None, 0, None, pk, pv, st),
        hip.flow_region_moments(m, None, fp, 0.25, pa, None, 0, None, pk, pv, st),
        hip.flow_region_moments(m, s, None, 0.25, pa, None, 0, None, pk, pv, st),
        hip.flow_region_moments(m, s, fp, 0.25, None, None, 0, None, pk, pv, st),
        hip.flow_region_moments(m, s, fp, 0.25, pa, None, 0, None, pk, None, st),
        hip.flow_region_moments(m, s, fp, 0.25, pa, None, 3, None, pk, pv, st),
        hip.flow_region_moments(m, s, fp, 0.25, pa, None, 1, fp, pk, pv, st),
        hip.flow_region_moments(m, s, fp, 0.25, pa, s, 1, None, pk, pv, st),
        hip.flow_region_moments(m, s, fp, 0.25, pa, ctypes.byref(cubic), 1, fp, pk, pv,
                                st),
        hip.flow_region_segment_sum(-1, pa, pb, 3, 4 * nc, pv, po, st),
        hip.flow_region_segment_sum(2, None, pb, 3, 4 * nc, pv, po, st),
        hip.flow_region_segment_sum(2, pa, None, 3, 4 * nc, pv, po, st),
        hip.flow_region_segment_sum(2, pa, pb, 3, 4 * nc, None, po, st),
        hip.flow_region_segment_sum(2, pa, pb, 3, 4 * nc, pv, None, st),
        hip.flow_region_segment_sum(2, pa, pb, 3, -1, pv, po, st),
        hip.flow_region_segment_minmax(-1, pa, pb, 1, N, fp, po, pv, st),
        hip.flow_region_segment_minmax(2, None, pb, 1, N, fp, po, pv, st),
        hip.flow_region_segment_minmax(2, pa, pb, 1, N, fp, None, pv, st),
        hip.flow_region_segment_minmax(2, pa, pb, 1, N, fp, po, po, st)]
    assert refused == [2] * len(refused)
    assert hip.flow_region_segment_sum(0, None, None, 3, 4 * nc, None, None, st) == 0
    assert hip.flow_region_segment_minmax(0, None, None, 1, N, None, None, None, st) == 0
    assert _hip.launch_count() == launches


def test_labels_that_are_no_iterate_become_outside(hip):
    '''A label buffer with entries that name no dof or a larger dof, passed
    straight to the entry point: those dofs are written as -1 and nothing
    outside the arrays is read (region_sweep_kernel tests a label against
    [0, i] before it uses it as an index).'''
    V = _space('square 12x11', 1)
    N = V.N
    start = numpy.arange(N, dtype=numpy.int32)
    start[5] = N + 1000            # past the end
    start[40] = 41                 # larger than the dof
    start[100] = -1                # outside
    a = device.to_device(start)
    b = torch.full_like(a, -7)
    flag = torch.zeros(1, dtype=torch.int32, device=device.get())
    _hip.check(hip.flow_region_sweeps(
        ctypes.byref(ops.mesh_struct(V.mesh())), ctypes.byref(ops.space_struct(V.layout)),
        1, _hip.i32(a, N), _hip.i32(b, N), _hip.i32(flag, 1), _hip.stream()))
    got = host(b)
    assert got[5] == -1 and got[40] == -1 and got[100] == -1
    assert ((got >= -1) & (got <= numpy.arange(N))).all()
