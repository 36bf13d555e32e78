# -*- coding: utf-8 -*-
'''
fem.Transfer without a GPU: the same-mesh tables, the facet grid's ring
search against the brute force of tests/transfer_reference.py, the refusals
(all raised before the device is touched) and the ABI.

The coarse channel here is karman_channel(28, fitted=True): the smallest
fitted channel the generator builds (24 fails its blend-zone assertion).
'''
import numpy
import pytest

from flow_amd import fem
from flow_amd.fem import Transfer, transfer

import point_reference as pref
import transfer_reference as tref


def _space(mesh, deg, dim):
    return fem.FunctionSpace(mesh, 'CG', deg, dim=dim)


@pytest.mark.parametrize('deg_to', [1, 2])
@pytest.mark.parametrize('deg_from', [1, 2])
@pytest.mark.parametrize('kind', ['square', 'channel'])
def test_same_mesh_tables(kind, deg_from, deg_to):
    mesh = fem.UnitSquareMesh(3, 2) if kind == 'square' \
        else fem.karman_channel(28, fitted=True)
    lay_from = _space(mesh, deg_from, 1).layout
    lay_to = _space(mesh, deg_to, 1).layout
    cells, bary = transfer.same_mesh_table(lay_from, lay_to)
    assert cells.dtype == numpy.int32 and cells.shape == (lay_to.N,)
    assert bary.shape == (3, lay_to.N) and bary.flags['C_CONTIGUOUS']
    # the lowest-index cell that holds the node: the brute force's answer
    assert numpy.array_equal(cells, pref.locate(mesh, lay_to.dof_coords))
    # and, by the dof map alone: no lower cell lists the node
    for d in range(lay_to.N):
        holds = numpy.nonzero((lay_to.cell_dofs == d).any(axis=1))[0]
        assert holds[0] == cells[d]
    assert numpy.isin(bary, [0.0, 0.5, 1.0]).all()
    assert numpy.array_equal(bary.sum(axis=0), numpy.ones(lay_to.N))
    # the coordinates put the node where it is
    v = mesh.points[mesh.cell_vertices[cells]]                  # (n, 3, 2)
    x = numpy.einsum('kn,nkd->nd', bary, v)
    assert numpy.abs(x - lay_to.dof_coords).max() <= 1e-15


@pytest.mark.parametrize('dim', [1, 2])
def test_same_mesh_transfer_object(dim):
    '''A same-mesh Transfer needs no device: found everywhere, distance 0.'''
    mesh = fem.UnitSquareMesh(3, 2)
    T = Transfer(_space(mesh, 2, dim), _space(mesh, 1, dim))
    assert T.found.all() and T.found.dtype == bool
    assert numpy.array_equal(T.distance, numpy.zeros(mesh.num_vertices()))
    assert T.cells.dtype == numpy.int32
    assert numpy.array_equal(T.cells, pref.locate(mesh, mesh.points))


def test_facet_grid_rings_hold_the_nearest_facet():
    mesh = fem.karman_channel(28, fitted=True)
    g = transfer.facet_grid(mesh)
    assert g is transfer.facet_grid(mesh)
    nf = len(mesh.bfacets)
    assert g.cells.dtype == numpy.int32 and g.start.dtype == numpy.int32
    assert g.start[0] == 0 and g.start[-1] == len(g.cells)
    assert g.cells.min() >= 0 and g.cells.max() < nf
    # every facet is listed, ascending within a bucket
    assert len(numpy.unique(g.cells)) == nf
    for b in range(g.nx * g.ny):
        c = g.candidates(b)
        assert (numpy.diff(c) > 0).all()
    cx, cy, rad = mesh.hole
    rng = numpy.random.RandomState(3)
    ang = rng.uniform(0, 2 * numpy.pi, 60)
    in_hole = numpy.stack([cx + rad * rng.uniform(0, 0.97, 60) * numpy.cos(ang),
                           cy + rad * rng.uniform(0, 0.97, 60) * numpy.sin(ang)], axis=1)
    far = numpy.array([[-0.3, 0.0], [0.9, 0.2], [0.3, -0.5], [5.0, 5.0],
                       [-1.0, -1.0], [0.1, 0.3]])
    pts = numpy.concatenate([pref.random_points(mesh, 300, seed=5, margin=0.2),
                             in_hole, far, [[cx, cy]], mesh.points[::11]])
    cells = pref.locate(mesh, pts)
    assert (cells < 0).sum() > 100 and (cells >= 0).sum() > 100
    want, want_t, want_d = tref.nearest_facets(mesh, pts)
    fewer = 0
    for i, p in enumerate(pts):
        cand = g.search(p, tref.distance2_of(mesh, p))
        assert want[i] in cand
        got, t, d = tref.nearest_facets(mesh, p[None], facets=cand)
        assert got[0] == want[i] and t[0] == want_t[i] and d[0] == want_d[i]
        fewer += len(cand) < nf
    # the grid narrows: most points see a part of the boundary only
    assert fewer > len(pts) // 2


def test_nearest_facet_reference_by_hand():
    '''The restatement itself on a case with known answers.'''
    mesh = fem.UnitSquareMesh(2, 2)
    pts = numpy.array([[0.25, -0.5], [1.5, 1.5], [-0.25, 0.3], [0.5, 2.0]])
    f, t, d = tref.nearest_facets(mesh, pts)
    a, b = tref.facet_segments(mesh)
    foot = a[f] + t[:, None] * (b[f] - a[f])
    assert numpy.allclose(foot, [[0.25, 0.0], [1.0, 1.0], [0.0, 0.3], [0.5, 1.0]])
    assert numpy.allclose(d, [0.5, numpy.sqrt(0.5), 0.25, 1.0])
    # (0.5, 2.0) is as near to two facets, through their shared vertex: the
    # lower index wins
    d2, _ = tref.segment_distance2(a, b, pts[3:4])
    tie = numpy.nonzero(d2[0] == d2[0].min())[0]
    assert len(tie) == 2 and f[3] == tie[0]
    tab = tref.Table(mesh, pts)
    assert not tab.found.any()
    assert numpy.array_equal(tab.cells, mesh.bfacet_cell[f])
    assert (tab.bary >= 0).all() and (tab.bary <= 1).all()
    assert (tab.bary[mesh.bfacet_local[f], numpy.arange(4)] == 0).all()


def test_refusals(monkeypatch):
    mesh = fem.UnitSquareMesh(4, 4)
    other = fem.UnitSquareMesh(4, 4)
    P1, P2 = _space(mesh, 1, 1), _space(mesh, 2, 1)
    W = _space(mesh, 2, 2)
    mixed = fem.FunctionSpace(
        mesh, fem.VectorElement('CG', 'triangle', 2)
        * fem.FiniteElement('CG', 'triangle', 1))
    for a, b in ((W.sub(0), P2), (P2, W.sub(1)), (mixed, P2), (W, mixed)):
        with pytest.raises(NotImplementedError):
            Transfer(a, b)
    for a, b in ((W, P2), (P1, W)):
        with pytest.raises(ValueError, match='component'):
            Transfer(a, b)
    T = Transfer(P2, P1)
    for bad in (fem.Function(P1), fem.Function(W),
                fem.Function(_space(other, 2, 1)), 3.0, fem.Constant(1.0)):
        with pytest.raises(ValueError, match='u_from'):
            T.apply(bad)
    with pytest.raises(ValueError, match='out'):
        T.apply(fem.Function(P2), out=fem.Function(P2))
    w = fem.Function(P1)
    with pytest.raises(TypeError):
        w.interpolate(3.0)
    from flow_amd import parallel
    monkeypatch.setattr(parallel, 'active', lambda: True)
    for call in (lambda: Transfer(P2, P1), lambda: T.apply(fem.Function(P2)),
                 lambda: fem.interpolate(fem.Function(P2), P1),
                 lambda: w.interpolate(fem.Function(P2))):
        with pytest.raises(NotImplementedError, match='on strips'):
            call()


def test_abi():
    from flow_amd import _hip
    lib = _hip.load_library()
    assert lib.flow_abi_version() == 30
    for name in ('flow_nearest_cells', 'flow_transfer_apply'):
        assert name in _hip.SYMBOLS
        assert getattr(lib, name) is not None
