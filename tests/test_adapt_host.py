# -*- coding: utf-8 -*-
'''
Adaptive refinement without a GPU (flow_amd/fem/adapt.py): the neighbour
topology, refine() on three mesh families, mark(), the numpy evaluator of
the jump indicator (tests/adapt_reference.py) on closed forms, the refusals
(all raised before the device is touched), the ABI, and the adaptive Poisson
loop with the reference indicator and the host's sparse LU.

Orientation.  The generators' meshes hold cells of both orientations (the
two triangles of a 'right' quad are listed with opposite signs), so "keeps
the orientation" is asserted per cell: a child's signed area has its
parent's sign.

Angles.  Longest-edge / 4T-LE refinement never produces an angle below half
the smallest angle of the initial mesh; six adaptive passes here measure a
ratio of 1.0 on every diagonal pattern and on the perturbed mesh (printed).
'''
import math

import numpy
import pytest

from flow_amd import fem
from flow_amd.fem import adapt, JumpIndicator, mark, refine

import adapt_reference as aref

DIAGONALS = aref.DIAGONALS


def _signed(mesh):
    return adapt._signed_areas(mesh.points, mesh.cell_vertices)


def _perturbed(diagonal='right', seed=4):
    mesh = fem.UnitSquareMesh(4, 3, diagonal)
    p = mesh.points.copy()
    inside = (p[:, 0] > 0) & (p[:, 0] < 1) & (p[:, 1] > 0) & (p[:, 1] < 1)
    rng = numpy.random.RandomState(seed)
    p[inside] += rng.uniform(-0.06, 0.06, (int(inside.sum()), 2))
    return fem.Mesh(p, mesh.cell_vertices)


def _families():
    out = [('square ' + d, fem.UnitSquareMesh(4, 3, d)) for d in DIAGONALS]
    out.append(('perturbed', _perturbed()))
    out.append(('staircase hole', fem.rectangle_with_hole(
        0.0, 1.0, 0.0, 0.5, (0.4, 0.25), 0.12, 12, 6)))
    out.append(('fitted hole', fem.karman_channel(28, fitted=True)))
    return out


def _markers(mesh):
    nc = mesh.num_cells()
    one = numpy.zeros(nc, dtype=bool)
    one[nc // 3] = True
    rng = numpy.random.RandomState(7)
    return [('none', numpy.zeros(nc, dtype=bool)), ('all', None),
            ('one', one), ('random', rng.uniform(size=nc) < 0.3)]


def _min_angle(mesh):
    p = mesh.points[mesh.cell_vertices]
    best = math.pi
    for i in range(3):
        a = p[:, (i + 1) % 3] - p[:, i]
        b = p[:, (i + 2) % 3] - p[:, i]
        cos = (a * b).sum(axis=1) / numpy.hypot(*a.T) / numpy.hypot(*b.T)
        best = min(best, float(numpy.arccos(numpy.clip(cos, -1, 1)).min()))
    return best


# -- cell_neighbors -------------------------------------------------------------
@pytest.mark.parametrize('kind', ['square', 'graded'])
def test_cell_neighbors(kind):
    mesh = fem.UnitSquareMesh(3, 2) if kind == 'square' \
        else fem.karman_channel_graded(0.02)
    nb = mesh.cell_neighbors
    nc = mesh.num_cells()
    assert nb.shape == (nc, 3) and nb.dtype == numpy.int32
    assert nb.min() >= -1 and nb.max() < nc
    c, i = numpy.nonzero(nb >= 0)
    back = nb[nb[c, i]] == c[:, None]
    assert (back.sum(axis=1) == 1).all()
    # across facet i lies the cell that shares the edge opposite vertex i
    assert numpy.array_equal(mesh.cell_edges[c, i],
                             mesh.cell_edges[nb[c, i]][back])
    # -1 exactly on the boundary facets
    c, i = numpy.nonzero(nb < 0)
    got = set(zip(c.tolist(), i.tolist()))
    want = set(zip(mesh.bfacet_cell.tolist(), mesh.bfacet_local.tolist()))
    assert got == want and len(got) == len(mesh.bfacets)
    # the reference's own edge -> cells map agrees
    inner, pairs = aref.edge_cells(mesh)
    assert len(inner) == (nb >= 0).sum() // 2
    for a, b in ((0, 1), (1, 0)):
        assert (nb[pairs[:, a]] == pairs[:, b][:, None]).any(axis=1).all()


def test_facet_table_packs_neighbour_facet_and_direction():
    mesh = fem.karman_channel_graded(0.02)
    nc = mesh.num_cells()
    t = adapt.facet_table(mesh)
    assert t is adapt.facet_table(mesh)
    assert t.dtype == numpy.int32 and t.shape == (3 * nc,)
    t = t.reshape(3, nc).T
    assert numpy.array_equal(t < 0, mesh.cell_neighbors < 0)
    assert (t[t < 0] == -1).all()
    c, i = numpy.nonzero(t >= 0)
    n, j, flip = t[c, i] >> 3, (t[c, i] >> 1) & 3, t[c, i] & 1
    assert numpy.array_equal(n, mesh.cell_neighbors[c, i])
    v0 = numpy.array([1, 0, 0])
    v1 = numpy.array([2, 2, 1])
    cv = mesh.cell_vertices
    mine0, mine1 = cv[c, v0[i]], cv[c, v1[i]]
    theirs0, theirs1 = cv[n, v0[j]], cv[n, v1[j]]
    assert numpy.array_equal(numpy.where(flip == 0, theirs0, theirs1), mine0)
    assert numpy.array_equal(numpy.where(flip == 0, theirs1, theirs0), mine1)
    # an unstructured mesh meets every local facet on both sides, in most
    # pairings and in both directions (local facet 1 runs against the
    # other two)
    assert set(i.tolist()) == set(j.tolist()) == {0, 1, 2}
    assert len(set(zip(i.tolist(), j.tolist()))) >= 6
    assert set(flip.tolist()) == {0, 1}


# -- refine ---------------------------------------------------------------------
FAMILIES = dict(_families())


@pytest.mark.parametrize('name', sorted(FAMILIES))
def test_refine(name):
    mesh = FAMILIES[name]
    nc = mesh.num_cells()
    parent_area = _signed(mesh)
    for what, markers in _markers(mesh):
        fine = refine(mesh, markers)
        assert isinstance(fine, fem.Mesh)
        assert fine.vertex_origin is None and fine.cell_origin is None
        assert fine.hole == mesh.hole
        par = fine.parent_cell
        assert par.dtype == numpy.int64 and par.shape == (fine.num_cells(),)
        assert par.min() >= 0 and par.max() < nc
        # conforming: the topology builds (no edge with three cells), every
        # interior edge has two cells, and no vertex lies inside an edge
        _, pairs = aref.edge_cells(fine)
        assert len(pairs) + len(fine.bfacets) == fine.num_edges()
        assert 3 * fine.num_cells() == 2 * len(pairs) + len(fine.bfacets)
        em, _ = adapt.marked_edges(
            mesh, numpy.ones(nc, dtype=bool) if markers is None else markers)
        # the boundary grows by the split boundary edges only
        assert len(fine.bfacets) == len(mesh.bfacets) + em[mesh.bfacets].sum()
        assert fine.num_vertices() == mesh.num_vertices() + em.sum()
        # orientation kept, no degenerate child
        area = _signed(fine)
        assert (area * numpy.sign(parent_area)[par] > 0).all()
        # children fill their parents
        total = numpy.bincount(par, weights=numpy.abs(area), minlength=nc)
        diff = total - numpy.abs(parent_area)
        if mesh.hole is None:
            assert numpy.abs(diff).max() <= 1e-14 * numpy.abs(parent_area).max()
        else:
            cx, cy, rad = mesh.hole
            d = numpy.hypot(fine.points[:, 0] - cx, fine.points[:, 1] - cy)
            # the new vertices on the circle: not among the old points
            old = set(map(tuple, mesh.points))
            new = numpy.array([tuple(q) not in old for q in fine.points])
            snapped = new & (numpy.abs(d - rad) <= 1e-12 * rad)
            touched = numpy.zeros(nc, dtype=bool)
            touched[par[snapped[fine.cell_vertices].any(axis=1)]] = True
            scale = numpy.abs(parent_area).max()
            assert numpy.abs(diff[~touched]).max() <= 1e-14 * scale
            # the domain lies outside the circle: snapping outward shrinks
            assert (diff[touched] < 0).all()
            ends = mesh.points[mesh.edges[mesh.bfacets]] - numpy.array([cx, cy])
            on = numpy.abs(numpy.hypot(ends[:, :, 0], ends[:, :, 1]) - rad) \
                <= 1e-9 * rad
            split_hole = em[mesh.bfacets] & on.all(axis=1)
            assert snapped.sum() == split_hole.sum()
            assert touched.any() == split_hole.any()
            assert touched.sum() <= split_hole.sum()
        # every marked cell has children only; an unmarked, untouched one
        # stays
        count = numpy.bincount(par, minlength=nc)
        if markers is None:
            assert fine.num_cells() == 4 * nc and (count == 4).all()
        else:
            assert (count[markers] == 4).all()
            assert (count >= 1).all() and (count <= 4).all()
            if not markers.any():
                assert fine.num_cells() == nc
                assert numpy.array_equal(numpy.sort(par), numpy.arange(nc))
        # numbered as reordered() numbers: renumbering changes nothing
        again = fine.reordered()
        assert numpy.array_equal(again.points, fine.points)
        assert numpy.array_equal(again.cell_vertices, fine.cell_vertices)
        # ... and the bandwidth stays of the order of one cross-section of
        # vertices (the refined mesh has at most twice as many across)
        section = numpy.sqrt(fine.num_vertices())
        base = mesh.reordered().bandwidth()
        print('%s / %s: %d -> %d cells, bandwidth %d -> %d'
              % (name, what, nc, fine.num_cells(), base, fine.bandwidth()))
        assert fine.bandwidth() <= max(4 * base, 4 * section)


def test_refine_snaps_hole_midpoints_onto_the_circle():
    mesh = fem.karman_channel(28, fitted=True)
    cx, cy, rad = mesh.hole
    fine = refine(mesh)
    d = numpy.hypot(fine.points[:, 0] - cx, fine.points[:, 1] - cy)
    ring = fine.points[numpy.unique(fine.edges[fine.bfacets])]
    dr = numpy.hypot(ring[:, 0] - cx, ring[:, 1] - cy)
    on_hole = dr < 2.0 * rad
    # every boundary vertex at the hole lies on the circle: old ones and the
    # new midpoints alike
    assert on_hole.sum() >= 16
    assert numpy.abs(dr[on_hole] - rad).max() <= 1e-12 * rad
    assert d.min() >= rad * (1 - 1e-12)
    # twice: still on the circle, twice as many sides
    finer = refine(fine)
    ring2 = finer.points[numpy.unique(finer.edges[finer.bfacets])]
    dr2 = numpy.hypot(ring2[:, 0] - cx, ring2[:, 1] - cy)
    assert (dr2 < 2.0 * rad).sum() == 2 * on_hole.sum()
    assert numpy.abs(dr2[dr2 < 2.0 * rad] - rad).max() <= 1e-12 * rad


def test_refine_keeps_a_midpoint_on_the_chord_where_a_child_would_fold():
    '''Two cells on a "hole" whose chord is so long against the cell's
    height that the arc's midpoint lies beyond the opposite vertex.'''
    r = 1.0
    a = numpy.array([-math.sin(0.5), math.cos(0.5)])
    b = numpy.array([math.sin(0.5), math.cos(0.5)])
    top = numpy.array([0.0, 0.95])          # above the chord, below the arc
    far = numpy.array([0.0, 3.0])
    mesh = fem.Mesh(numpy.array([a, b, top, far, [2.0, 1.0], [-2.0, 1.0]]),
                    numpy.array([[0, 1, 2], [1, 4, 2], [2, 4, 3], [2, 3, 5],
                                 [0, 2, 5]], dtype=numpy.int32))
    mesh.hole = (0.0, 0.0, r)
    assert (_signed(mesh) > 0).all()
    fine = refine(mesh, numpy.array([True, False, False, False, False]))
    mid = 0.5 * (a + b)
    assert (numpy.abs(fine.points - mid).sum(axis=1) < 1e-15).any()
    assert (_signed(fine) > 0).all()


def test_refine_refusals():
    mesh = fem.UnitSquareMesh(3, 2)
    nc = mesh.num_cells()
    for bad in (numpy.zeros(nc + 1, dtype=bool), numpy.zeros((nc, 1), dtype=bool),
                numpy.zeros(nc, dtype=numpy.int32), numpy.zeros(nc),
                [0] * nc):
        with pytest.raises(ValueError, match='markers'):
            refine(mesh, bad)


@pytest.mark.parametrize('name', DIAGONALS + ('perturbed',))
def test_six_passes_keep_half_the_smallest_angle(name):
    mesh = _perturbed() if name == 'perturbed' else fem.UnitSquareMesh(4, 3, name)
    first = _min_angle(mesh)
    worst = first
    for _ in range(6):
        cen = mesh.points[mesh.cell_vertices].mean(axis=1)
        inside = numpy.hypot(cen[:, 0] - 0.6, cen[:, 1] - 0.45) < 0.2
        assert inside.any()
        mesh = refine(mesh, inside)
        worst = min(worst, _min_angle(mesh))
    print('%s: smallest angle %.4f -> %.4f rad over six passes (ratio %.4f), '
          '%d cells' % (name, first, worst, worst / first, mesh.num_cells()))
    assert worst >= 0.5 * first - 1e-12


# -- mark -----------------------------------------------------------------------
def test_mark_by_hand():
    eta = numpy.array([1.0, 8.0, 2.0, 8.0, 0.0, 4.0, 1.0])      # total 24
    m = mark(eta, 0.5)
    assert m.dtype == bool and m.shape == (7,)
    assert m.tolist() == [False, True, False, True, False, False, False]
    # ties fall by cell index: one of the two 8s is enough for a third
    assert mark(eta, 1.0 / 3.0).tolist() == [False, True] + [False] * 5
    assert mark(eta, 0.7).tolist() == [False, True, False, True, False, True,
                                       False]
    # everything: the zero is not needed
    assert mark(eta, 1.0).tolist() == [True, True, True, True, False, True, True]
    assert mark(eta, 0.5, 'maximum').tolist() == [False, True, False, True,
                                                  False, True, False]
    assert mark(eta, 1.0, 'maximum').tolist() == [False, True, False, True,
                                                  False, False, False]
    assert mark(eta, 0.2, 'fraction').tolist() == [False, True, False, True,
                                                   False, False, False]
    assert mark(eta, 0.1, 'fraction').tolist() == [False, True] + [False] * 5
    # the tie between the two 1s: the lower index
    assert mark(eta, 5.0 / 7.0, 'fraction').tolist() == [True, True, True, True,
                                                         False, True, False]
    assert mark(eta, 1.0, 'fraction').all()


def test_dorfler_set_is_minimal():
    rng = numpy.random.RandomState(11)
    for fraction in (0.1, 0.5, 0.9, 1.0):
        eta = rng.permutation(200).astype(float)        # exact sums
        m = mark(eta, fraction)
        chosen = numpy.sort(eta[m])[::-1]
        assert chosen.sum() >= fraction * eta.sum()
        assert chosen[:-1].sum() < fraction * eta.sum()
        # the largest ones
        assert chosen.min() >= eta[~m].max()
    # the same rules on a host tensor
    import torch
    eta = rng.permutation(300).astype(float)
    for strategy in adapt.STRATEGIES:
        assert numpy.array_equal(mark(torch.from_numpy(eta), 0.4, strategy),
                                 mark(eta, 0.4, strategy))


def test_mark_refusals():
    import torch
    eta = numpy.array([1.0, 2.0, 3.0])
    for fraction in (0.0, -0.1, 1.5, float('nan')):
        with pytest.raises(ValueError, match='fraction'):
            mark(eta, fraction)
    with pytest.raises(ValueError, match='strategy'):
        mark(eta, 0.5, 'bulk')
    bad = numpy.array([1.0, float('nan'), 3.0])
    for strategy in adapt.STRATEGIES:
        with pytest.raises(ValueError, match='NaN'):
            mark(bad, 0.5, strategy)
        with pytest.raises(ValueError, match='NaN'):
            mark(torch.from_numpy(bad), 0.5, strategy)
    with pytest.raises(ValueError):
        mark([1.0, 2.0], 0.5)
    with pytest.raises(ValueError):
        mark(numpy.ones((2, 2)), 0.5)


# -- the reference evaluator on closed forms -----------------------------------------
def test_reference_kink():
    mesh = fem.UnitSquareMesh(4, 4)
    u = aref.field(fem.FunctionSpace(mesh, 'CG', 1),
               [lambda x, y: numpy.abs(x - 0.5)])
    got = aref.indicator(u)
    want = aref.kink_expectation(mesh)
    assert (want > 0).sum() == 8
    assert numpy.abs(got - want)[want > 0].max() <= 1e-15
    assert numpy.abs(got[want == 0]).max() <= 1e-28


def test_reference_smooth_fields_have_no_jump():
    mesh = fem.UnitSquareMesh(4, 4, 'crossed')
    for deg, dim, funcs, gmax in aref.SMOOTH:
        u = aref.field(fem.FunctionSpace(mesh, 'CG', deg, dim=dim), funcs)
        assert numpy.abs(aref.indicator(u)).max() <= 1e-24 * gmax**2


# -- refusals, symbols, ABI ------------------------------------------------------
def test_refusals(monkeypatch):
    mesh = fem.UnitSquareMesh(4, 4)
    other = fem.UnitSquareMesh(4, 4)
    P1, P2 = fem.FunctionSpace(mesh, 'CG', 1), fem.FunctionSpace(mesh, 'CG', 2)
    W = fem.VectorFunctionSpace(mesh, 'CG', 2)
    mixed = fem.FunctionSpace(
        mesh, fem.VectorElement('CG', 'triangle', 2)
        * fem.FiniteElement('CG', 'triangle', 1))
    for V in (mixed, W.sub(0), W.sub(1)):
        with pytest.raises(NotImplementedError):
            JumpIndicator(V)

    class Cubic(object):
        layout, component, degree, dim = P2.layout, None, 3, 1

    with pytest.raises(ValueError, match='P3'):
        JumpIndicator(Cubic())
    J = JumpIndicator(P2)
    for bad in (fem.Function(P1), fem.Function(W),
                fem.Function(fem.FunctionSpace(other, 'CG', 2)), 3.0,
                fem.Constant(1.0)):
        with pytest.raises(ValueError, match='u:'):
            J.apply(bad)
    from flow_amd import parallel
    monkeypatch.setattr(parallel, 'active', lambda: True)
    for call in (lambda: JumpIndicator(P2), lambda: J.apply(fem.Function(P2)),
                 lambda: J.estimate(fem.Function(P2)),
                 lambda: fem.jump_indicator(fem.Function(P1))):
        with pytest.raises(NotImplementedError, match='on strips'):
            call()


def test_abi():
    from flow_amd import _hip
    lib = _hip.load_library()
    assert lib.flow_abi_version() == 30
    assert 'flow_jump_indicator' in _hip.SYMBOLS
    assert getattr(lib, 'flow_jump_indicator') is not None


# -- the adaptive loop on the host -------------------------------------------------
def test_adaptive_loop_beats_uniform_refinement():
    '''-laplace u = f, P1, a Gaussian bump of width SIGMA: after CYCLES
    cycles of reference indicator -> mark(FRACTION, 'dorfler') -> refine the
    L2 error is below that of the coarsest uniformly refined mesh with at
    least as many dofs.'''
    mesh = fem.UnitSquareMesh(8, 8)
    rows = []
    for cycle in range(aref.CYCLES + 1):
        V, x = aref.host_solve(mesh)
        rows.append((V.N, aref.l2_error(V, x)))
        if cycle == aref.CYCLES:
            break
        u = fem.Function(V)
        u.set_array(x)
        mesh = refine(mesh, mark(aref.indicator(u), aref.FRACTION, 'dorfler'))
    uniform = aref.uniform_errors(aref.host_solve, rows[-1][0],
                                  fem.UnitSquareMesh(8, 8))
    print('adaptive: %s' % rows)
    print('uniform:  %s' % uniform)
    n, e = aref.uniform_error_for(rows[-1][0], uniform)
    assert n >= rows[-1][0]
    assert rows[-1][1] < e
