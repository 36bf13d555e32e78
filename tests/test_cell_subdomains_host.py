# -*- coding: utf-8 -*-
'''
Cell subdomains, dx(k), on the host (no device): the switch, the measure's
spellings and refusals, SubDomain.mark on a cell MeshFunction, the cell
contribution map (ops.cell_map_host) for every selection of
tests/test_cell_subdomains_gpu.py, derivative / lhs / rhs, refined_markers and
the jobs of the Newton assembler.
'''
import numpy
import pytest

from flow_amd import fem
from flow_amd.fem import (
    TestFunction, TrialFunction, dx, ds, Measure, MeshFunction, CellFunction,
    inner, grad, lhs, rhs, derivative,
    )
from flow_amd.fem import forms, ops

KBLOCK = 256            # csrc/common.h
NOTHING = 99


@pytest.fixture
def on():
    with fem.cell_subdomains(True):
        yield


class Disc(fem.SubDomain):
    '''A disc whose circle cuts across cells.'''

    def __init__(self, cx, cy, r):
        fem.SubDomain.__init__(self)
        self.c = (cx, cy, r)

    def inside(self, x, on_boundary):
        cx, cy, r = self.c
        return (x[0] - cx)**2 + (x[1] - cy)**2 < r * r


def selections(mesh, disc):
    '''[(name, markers, id)]: a disc, the first kBlock + 1 cells, one cell,
    all cells, nobody.'''
    nc = mesh.num_cells()
    geo = MeshFunction('size_t', mesh, 2, 0)
    disc.mark(geo, 1)
    first = MeshFunction('size_t', mesh, 2, 0)
    first.set_where(numpy.arange(nc) < KBLOCK + 1, 2)
    one = MeshFunction('size_t', mesh, 2, 0)
    one[nc // 3] = 3
    everything = CellFunction('size_t', mesh, 4)
    return [('disc', geo, 1), ('first', first, 2), ('one', one, 3),
            ('all', everything, 4), ('nothing', geo, NOTHING)]


def cases():
    sq = fem.UnitSquareMesh(12, 9)
    ch = fem.karman_channel(60, 14, fitted=True)
    xmax, ymax = ch.points.max(axis=0)
    return [('square', sq, selections(sq, Disc(0.4, 0.55, 0.3))),
            ('channel', ch, selections(ch, Disc(0.3 * xmax, 0.5 * ymax,
                                                0.45 * ymax)))]


def test_switch():
    mesh = fem.UnitSquareMesh(2, 2)
    assert fem.cell_subdomains.enabled is False
    with pytest.raises(NotImplementedError):
        dx(1)
    with pytest.raises(NotImplementedError):
        MeshFunction('size_t', mesh, 2)
    with pytest.raises(NotImplementedError):
        CellFunction('size_t', mesh)
    with fem.cell_subdomains(True) as s:
        assert s.previous is False and fem.cell_subdomains.enabled is True
        assert MeshFunction('size_t', mesh, 2).size() == mesh.num_cells()
        with fem.cell_subdomains(False):
            with pytest.raises(NotImplementedError):
                dx(1)
        assert fem.cell_subdomains.enabled is True
    assert fem.cell_subdomains.enabled is False
    with pytest.raises(NotImplementedError):
        dx(subdomain_data=object())
    assert forms.cell_subdomains is fem.cell_subdomains
    assert issubclass(forms.cell_subdomains, forms._Switch)


def test_cell_mesh_function(on):
    mesh = fem.UnitSquareMesh(3, 2)
    m = MeshFunction('size_t', mesh, 2, 7)
    assert m.dim == 2 and m.size() == mesh.num_cells() == 12
    assert (m.array() == 7).all() and not m.array().flags.writeable
    v = m.version
    m.set_all(1)
    m[3] = 5
    m.set_where(numpy.arange(12) >= 10, 2)
    assert m.version == v + 3
    assert list(m.array()) == [1, 1, 1, 5, 1, 1, 1, 1, 1, 1, 2, 2]
    assert m[3] == 5
    c = CellFunction('int', mesh, 4)
    assert c.dim == 2 and (c.array() == 4).all()
    # the facet kind is what it was
    assert MeshFunction('size_t', mesh, 1).size() == mesh.num_edges()


def test_measure(on):
    mesh = fem.UnitSquareMesh(4, 4)
    other = fem.UnitSquareMesh(4, 4)
    V = fem.FunctionSpace(mesh, 'CG', 1)
    v = TestFunction(V)
    m = MeshFunction('size_t', mesh, 2, 0)
    facets = MeshFunction('size_t', mesh, 1, 0)
    dxm = Measure('dx', domain=mesh, subdomain_data=m)
    for d, k in ((dxm(1), 1), (dxm(subdomain_id=2), 2),
                 (dx(3, subdomain_data=m), 3),
                 (dx(subdomain_data=m)(4), 4),
                 (dx(subdomain_id=5, subdomain_data=m, degree=3), 5)):
        f = v * d
        assert f.integral_type == 'cell' and f.subdomain_id == k
        assert f.subdomain_data is m and f.mesh is mesh
        assert ops.is_cell_subdomain(f)
    f = v * dx(subdomain_data=m)
    assert f.subdomain_id == 'everywhere' and not ops.is_cell_subdomain(f)
    assert not ops.is_cell_subdomain(v * dx)
    # the mesh may come from the markers
    f = 1.0 * dxm(1)
    assert f.mesh is mesh
    assert (2.0 * dx(1, subdomain_data=m)).mesh is mesh
    # dx(k) without markers: the ValueError ds(k) gives
    with pytest.raises(ValueError, match='needs markers'):
        ops.cell_lists(mesh, None, 1)
    with pytest.raises(ValueError, match='needs markers'):
        ops.facet_lists(mesh, None, 1)
    with pytest.raises(ValueError, match='another mesh'):
        v * dx(1, subdomain_data=MeshFunction('size_t', other, 2, 0))
    with pytest.raises(ValueError, match='another mesh'):
        ops.cell_lists(mesh, MeshFunction('size_t', other, 2, 0), 1)
    with pytest.raises(ValueError, match='cell MeshFunction'):
        dx(1, subdomain_data=facets)
    with pytest.raises(ValueError, match='facet MeshFunction'):
        ds(1, subdomain_data=m)
    with pytest.raises(ValueError, match='facet MeshFunction'):
        Measure('ds', domain=mesh, subdomain_data=m)
    with fem.interior_facets(True):
        with pytest.raises(ValueError, match='facet MeshFunction'):
            fem.dS(1, subdomain_data=m)
    with pytest.raises(ValueError, match='one integer'):
        dxm((1, 2))
    with pytest.raises(ValueError, match='one integer'):
        dxm(1.5)


def test_mark_against_brute_force(on):
    for tag, mesh, sels in cases():
        name, m, k = sels[0]
        disc = Disc(*(
            (0.4, 0.55, 0.3) if tag == 'square' else
            (0.3 * mesh.points[:, 0].max(), 0.5 * mesh.points[:, 1].max(),
             0.45 * mesh.points[:, 1].max())))
        want = numpy.zeros(mesh.num_cells(), dtype=bool)
        cut = 0
        for c, vs in enumerate(mesh.cell_vertices):
            p = mesh.points[vs]
            pts = list(p) + [p.mean(axis=0)]
            inside = [bool(disc.inside(x, False)) for x in pts]
            want[c] = all(inside)
            cut += any(inside) and not all(inside)
        got = m.array() == 1
        assert numpy.array_equal(got, want)
        # the circle cuts cells, and a cut cell stays unmarked
        assert cut > 0 and want.any() and not want.all()
        print('%s: %d cells in the disc, %d cut' % (tag, want.sum(), cut))
    # a later mark overrides, the version follows
    mesh = fem.UnitSquareMesh(4, 4)
    m = MeshFunction('size_t', mesh, 2, 0)
    v = m.version

    class Left(fem.SubDomain):
        def inside(self, x, on_boundary):
            assert on_boundary is False
            return x[0] <= 0.5 + 1e-12

    Left().mark(m, 6)
    assert m.version == v + 1
    mid = mesh.points[mesh.cell_vertices].mean(axis=1)
    assert numpy.array_equal(m.array() == 6, mid[:, 0] < 0.5)


def _decode(src, n):
    '''(ij, position) of scratch indices with stride n.'''
    return src // n, src % n


def test_cell_map_host(on):
    for tag, mesh, sels in cases():
        nc = mesh.num_cells()
        for V in (fem.FunctionSpace(mesh, 'CG', 1),
                  fem.FunctionSpace(mesh, 'CG', 2)):
            lay = V.layout
            for rank in (1, 2):
                if rank == 2:
                    sptr, ssrc = lay.pattern('cptr'), lay.pattern('csrc')
                else:
                    sptr, ssrc = lay.vmap('vptr'), lay.vmap('vsrc')
                for name, m, k in sels:
                    sel = numpy.nonzero(m.array() == k)[0]
                    nsel = len(sel)
                    targets, ptr, src = ops.cell_map_host(mesh, lay, rank, m, k)
                    assert targets.dtype == ptr.dtype == src.dtype \
                        == numpy.int32
                    if nsel == 0:
                        assert len(targets) == 0 and len(src) == 0 \
                            and list(ptr) == [0]
                        continue
                    # every scratch entry exactly once
                    assert numpy.array_equal(
                        numpy.sort(src), numpy.arange(lay.nloc**rank * nsel))
                    # sorted, unique targets; ptr is a partition
                    assert (numpy.diff(targets) > 0).all()
                    assert ptr[0] == 0 and ptr[-1] == len(src) \
                        and (numpy.diff(ptr) > 0).all() \
                        and len(ptr) == len(targets) + 1
                    if name == 'all' or nsel == nc:
                        # the space's own map, entry by entry
                        assert numpy.array_equal(src, ssrc)
                        assert numpy.array_equal(ptr, sptr[targets.tolist()
                                                           + [len(sptr) - 1]])
                        assert len(targets) == len(sptr) - 1
                        continue
                    # a partial selection: the space's sources, filtered
                    chosen = numpy.zeros(nc, dtype=bool)
                    chosen[sel] = True
                    for t in range(len(targets)):
                        tg = targets[t]
                        own = ssrc[sptr[tg]:sptr[tg + 1]].astype(numpy.int64)
                        own = own[chosen[own % nc]]
                        ij, pos = _decode(src[ptr[t]:ptr[t + 1]].astype(
                            numpy.int64), nsel)
                        assert numpy.array_equal(ij, own // nc)
                        assert numpy.array_equal(sel[pos], own % nc)
                    # ... and no other target has a selected source
                    has = numpy.zeros(len(sptr) - 1, dtype=bool)
                    has[targets] = True
                    count = numpy.add.reduceat(
                        chosen[ssrc % nc].astype(int), sptr[:-1])
                    assert numpy.array_equal(count > 0, has)


def test_derivative_lhs_rhs(on):
    mesh = fem.UnitSquareMesh(4, 4)
    V = fem.FunctionSpace(mesh, 'CG', 1)
    m = MeshFunction('size_t', mesh, 2, 0)
    dxm = Measure('dx', domain=mesh, subdomain_data=m)
    u, v = TrialFunction(V), TestFunction(V)
    w = fem.Function(V)
    F = (1 + w**2) * inner(grad(w), grad(v)) * dxm(1) \
        + inner(grad(w), grad(v)) * dxm(0) - v * dx
    J = derivative(F, w)
    parts = J.terms()
    assert [(p.subdomain_id, p.subdomain_data) for _, p in parts] \
        == [(1, m), (0, m)]
    assert all(p.integral_type == 'cell' and p.rank == 2 for _, p in parts)
    k0, k1 = fem.Constant(1.0), fem.Constant(10.0)
    f = fem.Constant(2.0)
    eq = k0 * inner(grad(u), grad(v)) * dxm(0) \
        + k1 * inner(grad(u), grad(v)) * dxm(1) - f * v * dxm(1) - v * dx
    a, L = lhs(eq), rhs(eq)
    assert [(s, p.subdomain_id) for s, p in a.terms()] == [(1.0, 0), (1.0, 1)]
    assert [(s, p.subdomain_id) for s, p in L.terms()] \
        == [(1.0, 1), (1.0, 'everywhere')]
    assert all(p.subdomain_data is m for _, p in a.terms())
    assert a.rank == 2 and L.rank == 1
    # sums and signs keep the parts as they are
    neg = -(u * v * dxm(1)) + u * v * dx - u * v * dxm(0)
    assert [(s, p.subdomain_id) for s, p in neg.terms()] \
        == [(-1.0, 1), (1.0, 'everywhere'), (-1.0, 0)]


def test_refined_markers(on):
    mesh = fem.UnitSquareMesh(6, 5)
    m = MeshFunction('size_t', mesh, 2, 0)
    Disc(0.5, 0.5, 0.35).mark(m, 1)
    m[0] = 7
    marked = numpy.zeros(mesh.num_cells(), dtype=bool)
    marked[::3] = True
    fine = fem.refine(mesh, marked)
    fm = fem.refined_markers(m, fine)
    assert fm.mesh is fine and fm.dim == 2 and fm.value_type == 'size_t'
    assert fm.size() == fine.num_cells() > mesh.num_cells()
    assert numpy.array_equal(fm.array(), m.array()[fine.parent_cell])
    # areas per material are kept
    def areas(msh, mm):
        p = msh.points[msh.cell_vertices]
        e, f = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
        a = 0.5 * numpy.abs(e[:, 0] * f[:, 1] - e[:, 1] * f[:, 0])
        return [a[mm.array() == k].sum() for k in (0, 1, 7)]
    assert numpy.allclose(areas(mesh, m), areas(fine, fm), rtol=1e-13)
    with pytest.raises(ValueError):
        fem.refined_markers(m, mesh)
    with pytest.raises(ValueError):
        fem.refined_markers(MeshFunction('size_t', mesh, 1, 0), fine)


def test_newton_jobs_by_parts(on):
    mesh = fem.UnitSquareMesh(4, 4)
    m = MeshFunction('size_t', mesh, 2, 0)
    dxm = Measure('dx', domain=mesh, subdomain_data=m)
    V = fem.FunctionSpace(mesh, 'CG', 2)
    v = TestFunction(V)
    w = fem.Function(V)
    F = (1 + w**2) * inner(grad(w), grad(v)) * dxm(1) \
        + inner(grad(w), grad(v)) * dxm(0) - v * dx
    J = derivative(F, w)
    jobs = ops.newton_jobs(J, F)
    assert [j.kind for j in jobs] == ['cells_matrix', 'cells_matrix',
                                      'cells_vector', 'cells_vector', 'vector']
    assert [j.part.subdomain_id for j in jobs[:4]] == [1, 0, 1, 0]
    assert jobs[4].part is None
    assert not ops._scalar_jobs_fused(jobs)
    # the whole-mesh form is still fused
    F0 = (1 + w**2) * inner(grad(w), grad(v)) * dx - v * dx
    jobs0 = ops.newton_jobs(derivative(F0, w), F0)
    assert [j.kind for j in jobs0] == ['newton', 'vector']
    assert ops._scalar_jobs_fused(jobs0)
    # a dx(k) part alone is not the fused single-dx case
    one = [(1.0, (v * dxm(1)))]
    assert not ops.NewtonAssembler._single_dx(one)
    assert ops.NewtonAssembler._single_dx([(1.0, v * dx)])


def test_caching_follows_the_version(on):
    mesh = fem.UnitSquareMesh(6, 4)
    lay = fem.FunctionSpace(mesh, 'CG', 1).layout
    m = MeshFunction('size_t', mesh, 2, 0)
    m.set_where(numpy.arange(mesh.num_cells()) % 4 == 0, 1)
    cells, n = ops.cell_lists(mesh, m, 1)
    assert n == 12 and cells.dtype == torch_int32()
    assert list(cells.cpu().numpy()) == list(range(0, 48, 4))
    again = ops.cell_lists(mesh, m, 1)
    assert again[0] is cells and again[1] == n
    cmap = ops.cell_map(mesh, lay, 2, m, 1)
    assert ops.cell_map(mesh, lay, 2, m, 1) is cmap
    assert ops.cell_map(mesh, lay, 1, m, 1) is not cmap
    host = ops.cell_map_host(mesh, lay, 2, m, 1)
    assert cmap[3] == len(host[0])
    for dev, ref in zip(cmap[:3], host):
        assert numpy.array_equal(dev.cpu().numpy(), ref)
    # re-marking re-selects
    m[1] = 1
    cells2, n2 = ops.cell_lists(mesh, m, 1)
    assert n2 == 13 and cells2 is not cells
    assert list(cells2.cpu().numpy())[:3] == [0, 1, 4]
    cmap2 = ops.cell_map(mesh, lay, 2, m, 1)
    assert cmap2 is not cmap and cmap2[3] >= cmap[3]
    # an empty selection holds no device array
    assert ops.cell_lists(mesh, m, NOTHING) == (None, 0)
    assert ops.cell_map(mesh, lay, 2, m, NOTHING) == (None, None, None, 0)


def torch_int32():
    import torch
    return torch.int32


def test_cell_lists_need_markers_of_cells(on):
    mesh = fem.UnitSquareMesh(3, 3)
    facets = MeshFunction('size_t', mesh, 1, 0)
    with pytest.raises(ValueError, match='cell MeshFunction'):
        ops.cell_map_host and ops.cell_map(mesh, fem.FunctionSpace(
            mesh, 'CG', 1).layout, 1, facets, 1)
    assert ops.cell_lists(mesh) == (None, mesh.num_cells())
    assert ops.cell_lists(mesh, None, 'everywhere') == (None, 18)
