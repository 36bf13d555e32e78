# -*- coding: utf-8 -*-
'''
Connected components of level sets without a GPU (flow_amd/fem/regions.py):
the refusals (all raised before the device is touched), the numpy / scipy
restatement (tests/regions_reference.py) against closed forms, the host helper
that turns sorted keys into segment offsets, the exports and the symbols.

Area convergence, measured here with the restatement: two discs of radius 0.17
round (0.27, 0.30) and (0.71, 0.66) as {f >= -r^2}, f = max_k -|x - c_k|^2 as
nodal values; the error of each disc's area against pi r^2 on nested meshes:

    P1  UnitSquareMesh(16) -> (32)   disc 0: 4.067e-03 -> 1.004e-03  ratio 4.049
                                     disc 1: 3.694e-03 -> 1.028e-03  ratio 3.595
    P2  UnitSquareMesh(8)  -> (16)   the same figures (the sub-triangulation
                                     of P2 on n cells is P1's on 2 n)

f is concave near the discs, so f_h <= f, the polygon lies inside the disc and
the error is second order with one sign: the test asks for a factor of 3.
'''
import importlib
import os

import numpy
import pytest
import torch

from flow_amd import fem

import regions_reference as rref
from regions_reference import Triangulation, hole_mesh, nodal

# (fem.regions is the function; the module it hides)
freg = importlib.import_module('flow_amd.fem.regions')

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# -- 1. refusals ---------------------------------------------------------------------
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
            fem.Regions(V)
    with pytest.raises(NotImplementedError):
        fem.regions(fem.Function(W), 0.0)
    with pytest.raises(ValueError, match='f:'):
        fem.regions(3.0, 0.0)

    class Cubic(object):
        layout, component, degree, dim = P2.layout, None, 3, 1

        def mesh(self):
            return mesh

    with pytest.raises(NotImplementedError, match='P3'):
        fem.Regions(Cubic())
    R = fem.Regions(P2)
    f = fem.Function(P2)
    for bad in (fem.Function(P1), fem.Function(W),
                fem.Function(fem.FunctionSpace(other, 'CG', 2)), 3.0):
        with pytest.raises(ValueError, match='f:'):
            R.label(bad, 0.0)
    for bad in (numpy.nan, numpy.inf, -numpy.inf, 'high', None, [0.0, 1.0]):
        with pytest.raises(ValueError, match='level'):
            R.label(f, bad)
        with pytest.raises(ValueError, match='level'):
            fem.regions(f, bad)
    for bad in ('inside', 'ABOVE', 0, None):
        with pytest.raises(ValueError, match='side'):
            R.label(f, 0.0, side=bad)
    empty = freg.Components(R, f, 0.0, 'above', 0, 8, None, None, None, None,
                            None, None, None, None, None)
    for call in (empty.integrate, empty.extrema):
        with pytest.raises(ValueError, match='another mesh'):
            call(fem.Function(fem.FunctionSpace(other, 'CG', 2)))
        with pytest.raises(ValueError, match='g:'):
            call(3.0)
    with pytest.raises(ValueError, match='dofs of V'):
        empty.extrema(fem.Function(P1))
    with pytest.raises(ValueError, match='k:'):
        empty.mask(0)
    from flow_amd import parallel
    monkeypatch.setattr(parallel, 'active', lambda: True)
    for call in (lambda: fem.Regions(P2), lambda: R.label(f, 0.0),
                 lambda: fem.regions(f, 0.0), lambda: empty.integrate(f),
                 lambda: empty.extrema(f)):
        with pytest.raises(NotImplementedError, match='on strips'):
            call()


def test_exports():
    for name in ('Regions', 'regions'):
        assert getattr(fem, name) is getattr(freg, name)
    assert freg.CHECK_EVERY >= 1 and freg.SIDES == {'above': 0, 'below': 1}


# -- 2. the restatement against closed forms -----------------------------------------
@pytest.mark.parametrize('deg', [1, 2])
def test_everything_inside_is_one_component(deg):
    mesh = fem.UnitSquareMesh(5, 4, 'crossed')
    V = fem.FunctionSpace(mesh, 'CG', deg)
    x = nodal(V, lambda x, y: x)
    r = rref.regions(V.layout, numpy.ones(V.N), 0.5, g=x, glayout=V.layout)
    assert r['count'] == 1 and (r['labels'] == 0).all() and r['root'].tolist() == [0]
    assert r['size'].tolist() == [V.N]
    assert abs(r['area'][0] - 1.0) <= 1e-13
    assert numpy.abs(r['centroid'][0] - 0.5).max() <= 1e-13
    assert abs(r['moments'][3, 0] - 0.5) <= 1e-13          # int x dx
    assert numpy.abs(r['scale'][0] - r['area']).max() <= 1e-13
    none = rref.regions(V.layout, numpy.ones(V.N), 0.5, side='below')
    assert none['count'] == 0 and (none['labels'] == -1).all()
    assert none['area'].shape == (0,) and none['centroid'].shape == (0, 2)


def _hole_polygon(mesh):
    '''The vertices of the hole's boundary, chained.'''
    p = mesh.points
    ends = mesh.edges[mesh.bfacets]
    box = (numpy.isin(p[:, 0], (0.0, 1.0)) | numpy.isin(p[:, 1], (0.0, 1.0)))
    ends = ends[~(box[ends[:, 0]] & box[ends[:, 1]])]
    nxt = {}
    for a, b in ends.tolist():
        nxt.setdefault(a, []).append(b)
        nxt.setdefault(b, []).append(a)
    assert all(len(v) == 2 for v in nxt.values())
    start = ends[0, 0]
    loop, prev = [start], None
    while True:
        a, b = nxt[loop[-1]]
        step = b if a == prev else a
        prev = loop[-1]
        if step == start:
            break
        loop.append(step)
    assert len(loop) == len(ends)
    return p[loop]


@pytest.mark.parametrize('deg', [1, 2])
def test_whole_mesh_with_a_hole(deg):
    mesh = hole_mesh()
    V = fem.FunctionSpace(mesh, 'CG', deg)
    r = rref.regions(V.layout, numpy.zeros(V.N), 0.0)
    hole = rref.polygon_area(_hole_polygon(mesh))
    print('P%d: area %.15f, 1 - hole %.15f' % (deg, r['area'][0], 1.0 - hole))
    assert 0.05 < hole < 0.2
    assert r['count'] == 1 and r['size'].tolist() == [V.N]
    assert abs(r['area'][0] - (1.0 - hole)) <= 1e-13


CENTRES, RADIUS = numpy.array([[0.27, 0.30], [0.71, 0.66]]), 0.17


def _discs(x, y):
    return numpy.max([-(x - c[0])**2 - (y - c[1])**2 for c in CENTRES], axis=0)


@pytest.mark.parametrize('deg,sizes', [(1, (16, 32)), (2, (8, 16))])
def test_two_discs_converge_at_second_order(deg, sizes):
    errs = []
    for n in sizes:
        V = fem.FunctionSpace(fem.UnitSquareMesh(n, n), 'CG', deg)
        r = rref.regions(V.layout, nodal(V, _discs), -RADIUS**2)
        assert r['count'] == 2
        # ids ascend with the smallest dof; which disc is which, by position
        order = numpy.argsort(r['centroid'][:, 0])
        assert numpy.abs(r['centroid'][order] - CENTRES).max() <= numpy.sqrt(2.0) / n
        errs.append(numpy.abs(r['area'][order] - numpy.pi * RADIUS**2))
    for k in range(2):
        print('P%d disc %d: %.3e -> %.3e, ratio %.3f (asked: 3)'
              % (deg, k, errs[0][k], errs[1][k], errs[0][k] / errs[1][k]))
        assert errs[1][k] < errs[0][k] / 3.0


VORTICES = [((0.2, 0.4), 1.0), ((0.4, 0.6), -1.0), ((0.6, 0.4), 1.0),
            ((0.8, 0.6), -1.0)]


def _street(x, y):
    return sum(s * numpy.exp(-((x - c[0])**2 + (y - c[1])**2) / 0.06**2)
               for c, s in VORTICES)


@pytest.mark.parametrize('deg,n', [(1, 24), (2, 12)])
def test_a_staggered_row_of_gaussian_vortices(deg, n):
    V = fem.FunctionSpace(fem.UnitSquareMesh(n, n), 'CG', deg)
    w = nodal(V, _street)
    h = numpy.sqrt(2.0) / n
    for side, level, sign in (('above', 0.5, 1.0), ('below', -0.5, -1.0)):
        r = rref.regions(V.layout, w, level, side=side, g=w, glayout=V.layout)
        want = numpy.array([c for c, s in VORTICES if s == sign])
        assert r['count'] == len(want) == 2
        order = numpy.argsort(r['centroid'][:, 0])
        dist = numpy.hypot(*(r['centroid'][order] - want).T)
        print('P%d %s: centroids off by %s, mesh width %.3e; circulation %s'
              % (deg, side, dist, h, r['moments'][3]))
        assert dist.max() <= h
        assert (sign * r['moments'][3] > 0.0).all()
        # a dof lies within 1 / 48 of a centre in x and in y: the peak is
        # sampled at exp(-2 / (48 * 0.06)^2) = 0.786 of its height or more
        assert (sign * (r['gmax'] if sign > 0 else r['gmin'])[0] > 0.78).all()


@pytest.mark.parametrize('deg', [1, 2])
def test_above_and_below_share_the_mesh(deg):
    mesh = hole_mesh()
    V = fem.FunctionSpace(mesh, 'CG', deg)
    f = nodal(V, lambda x, y: numpy.sin(3 * numpy.pi * x + 0.4)
              * numpy.cos(2 * numpy.pi * y - 0.3))
    tri = Triangulation(V.layout)
    up = rref.regions(V.layout, f, 0.25, tri=tri)
    down = rref.regions(V.layout, f, 0.25, side='below', tri=tri)
    total = mesh.cell_areas().sum()
    assert up['count'] >= 3 and down['count'] >= 1
    assert ((up['labels'] >= 0) != (down['labels'] >= 0)).all()
    print('P%d: %d + %d components, %.15f + %.15f = %.15f'
          % (deg, up['count'], down['count'], up['area'].sum(), down['area'].sum(),
             total))
    assert abs(up['area'].sum() + down['area'].sum() - total) <= 1e-13 * total


def test_a_p2_edge_does_not_join_its_vertices():
    '''Two vertices of one cell inside, every mid point outside: two
    components, two pieces in one cell.'''
    V = fem.FunctionSpace(fem.UnitSquareMesh(1, 1), 'CG', 2)
    f = numpy.zeros(V.N)
    f[V.layout.vertex_dofs[V.layout.mesh.cell_vertices[0, :2]]] = 1.0
    r = rref.regions(V.layout, f, 0.5)
    assert r['count'] == 2 and r['size'].tolist() == [1, 1]
    assert (r['area'] > 0.0).all()


# -- 3. sorted keys -> segments ------------------------------------------------------
def test_segment_offsets():
    keys = torch.tensor([-1, -1, 0, 0, 0, 2, 3, 3], dtype=torch.int32)
    off = freg.segment_offsets(keys, 4)
    assert off.dtype == torch.int32 and off.tolist() == [2, 5, 5, 6, 8]
    assert freg.segment_offsets(keys[2:], 4).tolist() == [0, 3, 3, 4, 6]
    assert freg.segment_offsets(torch.zeros(0, dtype=torch.int32), 0).tolist() == [0]
    assert freg.segment_offsets(torch.full((3,), -1, dtype=torch.int32), 0).tolist() == [3]
    shuffled = torch.tensor([3, -1, 0, 2, 0, -1, 3, 0], dtype=torch.int32)
    perm, off = freg._sorted_segments(shuffled, 4)
    assert perm.dtype == torch.int32
    assert perm.tolist() == [1, 5, 2, 4, 7, 3, 0, 6]      # stable
    assert off.tolist() == [2, 5, 5, 6, 8]


# -- 4. symbols ----------------------------------------------------------------------
NARGS = (('flow_region_init', 6), ('flow_region_sweeps', 7),
         ('flow_region_moments', 11), ('flow_region_segment_sum', 8),
         ('flow_region_segment_minmax', 9))


def test_symbols_declared_and_bound():
    from flow_amd import _hip
    with open(os.path.join(ROOT, 'include', 'flow_hip.h')) as f:
        header = f.read()
    lib = _hip.load_library()
    for name, nargs in NARGS:
        assert 'int %s(' % name in header
        assert len(_hip.SYMBOLS[name]) == nargs
        decl = header[header.index('int %s(' % name):]
        assert decl[:decl.index(';')].count(',') == nargs - 1
        assert getattr(lib, name) is not None
    with open(os.path.join(ROOT, 'flow_amd', 'csrc', 'Makefile')) as f:
        assert 'region_kernels.hip' in f.read()


def test_entry_points_check_their_arguments_before_anything_else():
    '''Refused calls return FLOW_INVALID without a device: the addresses
    below are never read.'''
    import ctypes
    from flow_amd import _hip
    lib = _hip.load_library()
    p, q, r = ctypes.c_void_p(4096), ctypes.c_void_p(8192), ctypes.c_void_p(12288)
    mesh = _hip.MeshS(10, p)
    space = _hip.SpaceS(2, 30, 100, p, p, p, p, p)
    count = _hip.launch_count()

    def variant(cls, base, **fields):
        s = cls.from_buffer_copy(base)
        for key, value in fields.items():
            setattr(s, key, value)
        return s

    def ref(s):
        return ctypes.byref(s) if s is not None else None

    refused = []
    bad_spaces = [None, variant(_hip.SpaceS, space, n=0),
                  variant(_hip.SpaceS, space, r1=1)]
    for s in bad_spaces:
        refused.append(lib.flow_region_init(ref(s), p, 0.0, 0, q, None))
    refused += [lib.flow_region_init(ref(space), None, 0.0, 0, q, None),
                lib.flow_region_init(ref(space), p, 0.0, 0, None, None),
                lib.flow_region_init(ref(space), p, float('nan'), 0, q, None),
                lib.flow_region_init(ref(space), p, float('inf'), 0, q, None),
                lib.flow_region_init(ref(space), p, 0.0, 2, q, None),
                lib.flow_region_init(ref(space), p, 0.0, -1, q, None)]
    bad_spaces += [variant(_hip.SpaceS, space, deg=3),
                   variant(_hip.SpaceS, space, deg=0),
                   variant(_hip.SpaceS, space, cell_dofs=None)]
    pairs = [(mesh, s) for s in bad_spaces] + [
        (None, space), (variant(_hip.MeshS, mesh, nc=0), space),
        (variant(_hip.MeshS, mesh, nc=2**31 // 6 + 1), space),
        (variant(_hip.MeshS, mesh, c1=1), space)]
    for m, s in pairs:
        refused.append(lib.flow_region_sweeps(ref(m), ref(s), 8, p, q, r, None))
        refused.append(lib.flow_region_moments(ref(m), ref(s), p, 0.0, q, None, 0,
                                               None, r, q, None))
    M, S = ref(mesh), ref(space)
    refused += [
        lib.flow_region_sweeps(M, ref(variant(_hip.SpaceS, space, vptr=None)), 8, p,
                               q, r, None),
        lib.flow_region_sweeps(M, ref(variant(_hip.SpaceS, space, vsrc=None)), 8, p,
                               q, r, None),
        lib.flow_region_sweeps(M, S, 0, p, q, r, None),
        lib.flow_region_sweeps(M, S, 8, None, q, r, None),
        lib.flow_region_sweeps(M, S, 8, p, None, r, None),
        lib.flow_region_sweeps(M, S, 8, p, q, None, None),
        lib.flow_region_sweeps(M, S, 8, p, p, r, None),
        lib.flow_region_moments(ref(variant(_hip.MeshS, mesh, xy=None)), S, p, 0.0, q,
                                None, 0, None, r, q, None),
        lib.flow_region_moments(M, S, None, 0.0, q, None, 0, None, r, q, None),
        lib.flow_region_moments(M, S, p, 0.0, None, None, 0, None, r, q, None),
        lib.flow_region_moments(M, S, p, 0.0, q, None, 0, None, r, None, None),
        lib.flow_region_moments(M, S, p, float('nan'), q, None, 0, None, r, q, None),
        lib.flow_region_moments(M, S, p, 0.0, q, None, 3, None, r, q, None),
        lib.flow_region_moments(M, S, p, 0.0, q, None, -1, None, r, q, None),
        lib.flow_region_moments(M, S, p, 0.0, q, None, 1, p, r, q, None),
        lib.flow_region_moments(M, S, p, 0.0, q, S, 1, None, r, q, None),
        lib.flow_region_moments(M, S, p, 0.0, q,
                                ref(variant(_hip.SpaceS, space, deg=3)), 1, p, r, q,
                                None),
        lib.flow_region_segment_sum(-1, p, q, 3, 40, r, p, None),
        lib.flow_region_segment_sum(2, p, q, -1, 40, r, p, None),
        lib.flow_region_segment_sum(2, p, q, 3, -1, r, p, None),
        lib.flow_region_segment_sum(2, p, q, 65536, 40, r, p, None),
        lib.flow_region_segment_sum(2, None, q, 3, 40, r, p, None),
        lib.flow_region_segment_sum(2, p, None, 3, 40, r, p, None),
        lib.flow_region_segment_sum(2, p, q, 3, 40, None, p, None),
        lib.flow_region_segment_sum(2, p, q, 3, 40, r, None, None),
        lib.flow_region_segment_sum(2, p, q, 3, 40, r, r, None),
        lib.flow_region_segment_minmax(-1, p, q, 1, 30, r, p, q, None),
        lib.flow_region_segment_minmax(2, p, q, 1, -1, r, p, q, None),
        lib.flow_region_segment_minmax(2, None, q, 1, 30, r, p, q, None),
        lib.flow_region_segment_minmax(2, p, None, 1, 30, r, p, q, None),
        lib.flow_region_segment_minmax(2, p, q, 1, 30, None, p, q, None),
        lib.flow_region_segment_minmax(2, p, q, 1, 30, r, None, q, None),
        lib.flow_region_segment_minmax(2, p, q, 1, 30, r, p, None, None),
        lib.flow_region_segment_minmax(2, p, q, 1, 30, r, p, p, None),
        lib.flow_region_segment_minmax(2, p, q, 1, 30, r, r, q, None)]
    assert refused == [2] * len(refused)
    with pytest.raises(ValueError, match='invalid argument'):
        _hip.check(2)
    # no component, no row: nothing to do
    assert lib.flow_region_segment_sum(0, None, None, 3, 40, None, None, None) == 0
    assert lib.flow_region_segment_sum(2, None, None, 0, 40, None, None, None) == 0
    assert lib.flow_region_segment_minmax(0, None, None, 1, 30, None, None, None,
                                          None) == 0
    assert _hip.launch_count() == count
