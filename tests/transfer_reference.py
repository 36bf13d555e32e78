# -*- coding: utf-8 -*-
'''
numpy restatement of fem.Transfer (flow_amd/fem/transfer.py): where every
target node sits in the source mesh and what the source field is there.  No
grid and no library:

  * location by brute force over all cells with the lowest-index rule
    (tests/point_reference.py);
  * for nodes in no cell, the nearest boundary facet by brute force over all
    of mesh.bfacets: smallest squared distance, ties to the lowest facet
    index.  The distance is written in the operation order of the kernel
    (csrc/transfer_kernels.hip: segment_distance2, which does not contract),
    so that ties are decided alike;
  * values through the reference basis (flow_amd/fem/reference.py: tabulate).

This is the reference of every tolerance in tests/test_transfer_gpu.py.
'''
import numpy

from flow_amd.fem import reference

import point_reference as pref


def facet_segments(mesh):
    '''(a, b), each (nf, 2): the end points of the boundary facets in the
    order of mesh.bfacets, a the owning cell's local vertex facet_v0(lf) and
    b its facet_v1(lf) (lf = 0: 1, 2; lf = 1: 0, 2; lf = 2: 0, 1).'''
    lf = mesh.bfacet_local
    v = mesh.cell_vertices[mesh.bfacet_cell]            # (nf, 3)
    va = numpy.where(lf == 0, 1, 0)
    vb = numpy.where(lf == 2, 1, 2)
    k = numpy.arange(len(lf))
    return mesh.points[v[k, va]], mesh.points[v[k, vb]]


def segment_distance2(a, b, pts):
    '''(d2, t), each (n, nf): squared distance of every point to every
    segment and the parameter of the clamped foot point a + t (b - a).'''
    dx, dy = (b[:, 0] - a[:, 0])[None, :], (b[:, 1] - a[:, 1])[None, :]
    qx = pts[:, 0, None] - a[None, :, 0]
    qy = pts[:, 1, None] - a[None, :, 1]
    den = dx * dx + dy * dy
    with numpy.errstate(invalid='ignore', divide='ignore'):
        s = (qx * dx + qy * dy) / den
    s = numpy.where(s >= 0.0, numpy.where(s <= 1.0, s, 1.0), 0.0)
    ex, ey = qx - s * dx, qy - s * dy
    return ex * ex + ey * ey, s


def nearest_facets(mesh, pts, facets=None, chunk=256):
    '''(facet (n,), t (n,), dist (n,)) of the nearest boundary facet of every
    point by brute force (over `facets` only, if given).'''
    pts = numpy.asarray(pts, dtype=float).reshape(-1, 2)
    a, b = facet_segments(mesh)
    ids = numpy.arange(len(a)) if facets is None else numpy.asarray(facets)
    a, b = a[ids], b[ids]
    f = numpy.empty(len(pts), dtype=numpy.int64)
    t = numpy.empty(len(pts))
    d = numpy.empty(len(pts))
    for k in range(0, len(pts), chunk):
        d2, s = segment_distance2(a, b, pts[k:k + chunk])
        j = numpy.argmin(d2, axis=1)        # the first minimum: lowest index
        r = numpy.arange(len(j))
        f[k:k + chunk] = ids[j]
        t[k:k + chunk] = s[r, j]
        d[k:k + chunk] = numpy.sqrt(d2[r, j])
    return f, t, d


def distance2_of(mesh, pt):
    '''facets -> their squared distances to the one point pt: what
    FacetGrid.search (flow_amd/fem/transfer.py) asks for.'''
    a, b = facet_segments(mesh)
    pt = numpy.asarray(pt, dtype=float).reshape(1, 2)
    return lambda facets: segment_distance2(a[facets], b[facets], pt)[0][0]


class Table(object):
    '''cells (n,), bary (3, n), found (n,), distance (n,), and for the nodes
    not found facet (n,; -1 where found): the restatement of what a Transfer
    across meshes holds.'''

    def __init__(self, mesh_from, pts):
        pts = numpy.asarray(pts, dtype=float).reshape(-1, 2)
        n = len(pts)
        self.cells = pref.locate(mesh_from, pts).astype(numpy.int64)
        self.found = self.cells >= 0
        self.bary = numpy.zeros((3, n))
        f = self.found
        self.bary[:, f] = pref.barycentric_own(mesh_from, pts[f], self.cells[f])
        self.distance = numpy.zeros(n)
        self.facet = numpy.full(n, -1, dtype=numpy.int64)
        out = numpy.nonzero(~f)[0]
        if len(out):
            facet, t, d = nearest_facets(mesh_from, pts[out])
            lf = mesh_from.bfacet_local[facet]
            self.facet[out] = facet
            self.cells[out] = mesh_from.bfacet_cell[facet]
            self.distance[out] = d
            self.bary[numpy.where(lf == 0, 1, 0), out] = 1.0 - t
            self.bary[numpy.where(lf == 2, 1, 2), out] = t
        self.cells = self.cells.astype(numpy.int32)


def table(V_from, V_to):
    return Table(V_from.mesh(), V_to.layout.dof_coords)


def evaluate(V_from, values, cells, bary):
    '''(dim, n): the field with dof array `values` (dim * N,) of V_from at
    barycentric bary (3, n) of cells (n,).'''
    U = numpy.asarray(values, dtype=float).reshape(V_from.dim, V_from.N)
    tab = reference.tabulate(V_from.degree, bary[1:].T)         # (n, nloc)
    dofs = V_from.layout.cell_dofs[cells]                       # (n, nloc)
    return numpy.einsum('anl,nl->an', U[:, dofs], tab)


def nodal(V, funcs):
    '''The dof array of the nodal interpolant of funcs (one per component).'''
    xy = V.layout.dof_coords
    assert len(funcs) == V.dim
    return numpy.concatenate([f(xy[:, 0], xy[:, 1]) for f in funcs])


def transfer(V_from, V_to, values, tab=None):
    '''The dof array on V_to of the field `values` of V_from.'''
    tab = tab or table(V_from, V_to)
    return evaluate(V_from, values, tab.cells, tab.bary).reshape(-1)


def boundary_node_share(V):
    '''Share of the nodes of V that lie on the boundary of its mesh.'''
    mesh, lay = V.mesh(), V.layout
    on = numpy.zeros(lay.N, dtype=bool)
    on[lay.vertex_dofs[numpy.unique(mesh.edges[mesh.bfacets].ravel())]] = True
    if lay.edge_dofs is not None:
        on[lay.edge_dofs[mesh.bfacets]] = True
    return on.mean()


def obstacle_facets(mesh, box):
    '''Indices into mesh.bfacets of the boundary facets strictly inside the
    outer box (x0, x1, y0, y1): the obstacle's.'''
    x0, x1, y0, y1 = box
    a, b = facet_segments(mesh)
    mid = 0.5 * (a + b)
    eps = 1e-9
    return numpy.nonzero((mid[:, 0] > x0 + eps) & (mid[:, 0] < x1 - eps)
                         & (mid[:, 1] > y0 + eps) & (mid[:, 1] < y1 - eps))[0]
