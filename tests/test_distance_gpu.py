# -*- coding: utf-8 -*-
'''
The wall distance on the HIP path (flow_amd/fem/distance.py; csrc/
distance_kernels.hip) against the numpy restatement of tests/
distance_reference.py.

Meshes: UnitSquareMesh(5, 3) (24 / 77 dofs: less than one block),
UnitSquareMesh(17, 13) (252 / 945 dofs: a ragged tail, and more than one
block for P2) with every exterior facet as source, and the small fitted-hole
channel of the form tests, karman_channel(60, 14, fitted=True), with the
obstacle as source.  P1 and P2 on each.

The bound.  max |d_gpu - d_ref| <= 1e-12 * the mesh's diameter: the two sides
evaluate the same expression tree (contraction is off in the kernel), a path
has at most a few hundred nodes and each update rounds by a few ulp of the
diameter.  Measured on the MI355X: 0 on all six cases (the same bits).

Every test prints what it measured next to its bound (pytest -s).
'''
import ctypes
import functools

import numpy
import pytest
import torch

from flow_amd import _hip, device, fem
from flow_amd.fem import assemble, distance as fdist, dx, ops

import distance_reference as dref
import form_reference as fref

pytestmark = pytest.mark.gpu

TOL = 1e-12
MESHES = ('square 5x3', 'square 17x13', 'channel')


class Left(fem.SubDomain):
    def inside(self, x, on_boundary):
        return on_boundary & (x[0] < 1e-12)


class Obstacle(fem.SubDomain):
    '''The boundary facets strictly inside the channel's box.'''

    def inside(self, x, on_boundary):
        return on_boundary & (1e-12 < x[0]) & (x[0] < 0.6 - 1e-12) \
            & (-0.07 + 1e-12 < x[1]) & (x[1] < 0.07 - 1e-12)


@functools.lru_cache(maxsize=None)
def _mesh(name):
    if name == 'channel':
        return fem.karman_channel(60, 14, fitted=True)
    return fem.UnitSquareMesh(*{'square 5x3': (5, 3), 'square 17x13': (17, 13)}[name])


def _sources(name):
    return Obstacle() if name == 'channel' else 'on_boundary'


@functools.lru_cache(maxsize=None)
def _case(name, deg, plane=False):
    '''(V, sources, reference d, reference sweeps), computed once.'''
    V = fem.FunctionSpace(_mesh(name), 'CG', deg)
    sources = Left() if plane else _sources(name)
    d, sweeps = dref.distance(V, fdist.source_dofs(V, sources))
    d.flags.writeable = False
    return V, sources, d, sweeps


def _batches(sweeps):
    '''The reference's count rounded up to a multiple of CHECK_EVERY.'''
    every = fdist.CHECK_EVERY
    return -(-sweeps // every) * every


# -- 1. against the restatement ---------------------------------------------------
@pytest.mark.parametrize('deg', [1, 2])
@pytest.mark.parametrize('name', MESHES)
def test_against_reference(hip, name, deg):
    V, sources, want, sweeps = _case(name, deg)
    D = fem.Distance(V, sources)
    d = D.apply()
    assert isinstance(d, fem.Function) and d.function_space().same_as(V)
    got = d.array()
    bound = TOL * dref.diameter(V.mesh())
    err = numpy.abs(got - want).max()
    lip = dref.lipschitz_excess(V, got)
    print('%s P%d: %d dofs, sweeps %d (reference %d), error %.2e  bound %.2e, '
          'Lipschitz 1 + %.1e' % (name, deg, V.N, D.sweeps, sweeps, err, bound,
                                  lip - 1.0))
    assert numpy.isfinite(got).all() and got.min() == 0.0
    assert (got[D.dofs] == 0.0).all()
    assert err <= bound
    assert D.sweeps == _batches(sweeps)
    assert lip <= 1.0 + 1e-12


# -- 2. a plane front is exact -----------------------------------------------------
@pytest.mark.parametrize('deg', [1, 2])
def test_plane_wave(hip, deg):
    V, sources, want, sweeps = _case('square 17x13', deg, plane=True)
    D = fem.Distance(V, sources)
    got = D.apply().array()
    err = numpy.abs(got - V.layout.dof_coords[:, 0]).max()
    print('P%d: |d - x| max %.2e (1e-13), sweeps %d (reference %d)'
          % (deg, err, D.sweeps, sweeps))
    assert err <= 1e-13
    assert D.sweeps == _batches(sweeps)


# -- 3. determinism, the spellings of the sources, out= ------------------------------
@pytest.mark.parametrize('deg', [1, 2])
@pytest.mark.parametrize('name', ['square 17x13', 'channel'])
def test_same_bits_twice_sources_as_dofs_and_out(hip, name, deg):
    V, sources, want, sweeps = _case(name, deg)
    D = fem.Distance(V, sources)
    a, b = D.apply(), D.apply()
    assert a.data.data_ptr() != b.data.data_ptr()
    assert numpy.array_equal(a.array(), b.array())
    # the sources as a dof array, and as a mask
    E = fem.Distance(V, D.dofs.copy())
    assert numpy.array_equal(E.apply().array(), a.array())
    assert E.sweeps == D.sweeps
    mask = numpy.zeros(V.N, dtype=bool)
    mask[D.dofs] = True
    assert torch.equal(fem.Distance(V, mask).apply().data, a.data)
    # into an existing Function
    out = fem.Function(V)
    out.data.fill_(-1.0)
    ptr = out.data.data_ptr()
    assert D.apply(out=out) is out and out.data.data_ptr() == ptr
    assert torch.equal(out.data, a.data)
    with pytest.raises(ValueError, match='out:'):
        D.apply(out=fem.Function(fem.FunctionSpace(V.mesh(), 'CG', 3 - deg)))
    # the one-off spelling
    assert torch.equal(fem.wall_distance(V, sources).data, a.data)


# -- 4. downstream -----------------------------------------------------------------
@pytest.mark.parametrize('deg', [1, 2])
def test_the_distance_is_a_form_operand(hip, deg):
    V, sources, want, _ = _case('channel', deg)
    mesh = V.mesh()
    d = fem.wall_distance(V, sources)
    ref = fem.Function(V)
    ref.set_array(numpy.array(want))
    got = assemble(d * dx(mesh))
    expected = fref.functional(ref * dx(mesh))
    print('P%d: int d dx = %.15e, host evaluator %.15e' % (deg, got, expected))
    assert abs(got - expected) <= 1e-12 * abs(expected)
    # ... and under a branch: the area within delta of the obstacle
    near = assemble(fem.conditional(fem.lt(d, 0.01), 1.0, 0.0) * dx(mesh))
    assert 0.0 < near < mesh.cell_areas().sum()


def test_grade_the_mesh_towards_the_obstacle(hip):
    '''The use: mark the cells within delta of the wall, refine them.'''
    V, sources, _, _ = _case('channel', 1)
    mesh = V.mesh()
    d = fem.wall_distance(V, sources).array()
    near = (d[V.layout.cell_dofs].min(axis=1) < 0.01).astype(float)
    cells = fem.mark(near, 1.0, 'maximum')
    assert cells.dtype == bool and 0 < cells.sum() < mesh.num_cells()
    assert numpy.array_equal(cells, near > 0.0)
    fine = fem.refine(mesh, cells)
    assert fine.num_cells() > mesh.num_cells()
    # on the finer mesh the field is computed anew
    Vf = fem.FunctionSpace(fine, 'CG', 1)
    df = fem.wall_distance(Vf, Obstacle()).array()
    assert numpy.isfinite(df).all() and df.min() == 0.0


# -- 5. the entry point refuses what it cannot run -----------------------------------
def test_argument_errors_launch_nothing(hip):
    V, _, _, _ = _case('square 5x3', 2)
    mesh_s = ops.mesh_struct(V.mesh())
    space_s = ops.space_struct(V.layout)
    a, b = device.empty(V.N), device.empty(V.N)
    flag = device.zeros(1, dtype=torch.int32)
    pa, pb, pf = _hip.f64(a, V.N), _hip.f64(b, V.N), _hip.i32(flag, 1)

    def variant(**fields):
        s = _hip.SpaceS.from_buffer_copy(space_s)
        for key, value in fields.items():
            setattr(s, key, value)
        return s

    strips = _hip.MeshS.from_buffer_copy(mesh_s)
    strips.c1 = 1
    no_xy = _hip.MeshS.from_buffer_copy(mesh_s)
    no_xy.xy = None
    good = (mesh_s, space_s, 4, pa, pb, pf)
    bad = [
        (mesh_s, variant(deg=3)) + good[2:],
        (mesh_s, variant(deg=0)) + good[2:],
        (mesh_s, variant(vptr=None)) + good[2:],
        (mesh_s, variant(vsrc=None)) + good[2:],
        (mesh_s, variant(cell_dofs=None)) + good[2:],
        (mesh_s, variant(r1=1)) + good[2:],
        (strips,) + good[1:],
        (no_xy,) + good[1:],
        (mesh_s, space_s, 0, pa, pb, pf),
        (mesh_s, space_s, 4, None, pb, pf),
        (mesh_s, space_s, 4, pa, None, pf),
        (mesh_s, space_s, 4, pa, pb, None),
        (mesh_s, space_s, 4, pa, pa, pf),
        ]
    count = _hip.launch_count()
    for m, s, n, x, y, f in bad:
        rc = hip.flow_distance_sweeps(ctypes.byref(m), ctypes.byref(s), n, x, y,
                                      f, _hip.stream())
        assert rc == 2
        with pytest.raises(ValueError, match='invalid argument'):
            _hip.check(rc)
    assert hip.flow_distance_sweeps(None, ctypes.byref(space_s), 4, pa, pb, pf,
                                    _hip.stream()) == 2
    assert hip.flow_distance_sweeps(ctypes.byref(mesh_s), None, 4, pa, pb, pf,
                                    _hip.stream()) == 2
    assert _hip.launch_count() == count
    # ... and runs what it can: 4 sweeps are 4 launches, the result in buf_a
    start = numpy.full(V.N, numpy.inf)
    start[fdist.source_dofs(V, 'on_boundary')] = 0.0
    a.copy_(torch.from_numpy(start))
    _hip.check(hip.flow_distance_sweeps(*(
        [ctypes.byref(mesh_s), ctypes.byref(space_s)] + list(good[2:])
        + [_hip.stream()])))
    assert _hip.launch_count() == count + 4
    g = dref.Graph(2, V.layout.cell_dofs,
                   V.mesh().points[V.mesh().cell_vertices])
    want = start
    for _ in range(4):
        want = g.sweep(want)
    assert numpy.array_equal(device.to_host(a).numpy(), want)
    assert int(device.to_host(flag)[0]) == 1
