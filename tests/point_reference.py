# -*- coding: utf-8 -*-
'''
numpy references for point evaluation (flow_amd/fem/points.py): the owning
cell of a point by brute force over all cells -- the rule of
flow_locate_points: the LOWEST-index cell whose barycentric coordinates are
all >= -1e-12, else -1 -- and the value of a P1 / P2 field at a point from
the reference basis (flow_amd/fem/reference.py: tabulate).  No grid and no
library.
'''
import numpy

from flow_amd.fem import reference

TOL = -1.0e-12


def barycentric_all(mesh, pts, cells):
    '''lambda (3, n, m) of pts (n, 2) on the cells (m,): the kernel's
    operation order (it does not contract), so ties on edges are decided
    alike.'''
    v = mesh.points[mesh.cell_vertices[cells]]          # (m, 3, 2)
    x0, x1, x2 = v[:, 0, 0], v[:, 1, 0], v[:, 2, 0]
    y0, y1, y2 = v[:, 0, 1], v[:, 1, 1], v[:, 2, 1]
    j00, j01, j10, j11 = x1 - x0, x2 - x0, y1 - y0, y2 - y0
    det = j00 * j11 - j01 * j10
    dx = pts[:, 0, None] - x0[None, :]
    dy = pts[:, 1, None] - y0[None, :]
    l1 = (j11 * dx - j01 * dy) / det
    l2 = (j00 * dy - j10 * dx) / det
    l0 = 1.0 - l1 - l2
    return numpy.stack([l0, l1, l2])


def locate(mesh, pts, chunk=512):
    '''The owning cell of every point (int32, -1 for none), brute force.'''
    pts = numpy.asarray(pts, dtype=float).reshape(-1, 2)
    nc = mesh.num_cells()
    out = numpy.full(len(pts), -1, dtype=numpy.int64)
    for c0 in range(0, nc, chunk):
        todo = numpy.nonzero(out < 0)[0]
        if not len(todo):
            break
        cells = numpy.arange(c0, min(nc, c0 + chunk))
        lam = barycentric_all(mesh, pts[todo], cells)
        hit = (lam >= TOL).all(axis=0)                  # (n, m)
        any_hit = hit.any(axis=1)
        first = numpy.argmax(hit, axis=1)
        out[todo[any_hit]] = cells[first[any_hit]]
    return out.astype(numpy.int32)


def field_values(u, pts, cells):
    '''Values of Function u at pts on their cells: (dim, n).'''
    V = u.function_space()
    lam = barycentric_own(V.mesh(), pts, cells)
    U = u.array().reshape(V.dim, V.N)
    dofs = V.layout.cell_dofs[cells]                    # (n, nloc)
    out = numpy.empty((V.dim, len(pts)))
    for i in range(len(pts)):
        tab = reference.tabulate(V.degree, [[lam[1, i], lam[2, i]]])[0]
        out[:, i] = U[:, dofs[i]].dot(tab)
    return out


def barycentric_own(mesh, pts, cells):
    '''lambda (3, n) of point i on cell i (the operation order of
    barycentric_all).'''
    v = mesh.points[mesh.cell_vertices[cells]]
    x0, x1, x2 = v[:, 0, 0], v[:, 1, 0], v[:, 2, 0]
    y0, y1, y2 = v[:, 0, 1], v[:, 1, 1], v[:, 2, 1]
    j00, j01, j10, j11 = x1 - x0, x2 - x0, y1 - y0, y2 - y0
    det = j00 * j11 - j01 * j10
    dx, dy = pts[:, 0] - x0, pts[:, 1] - y0
    l1 = (j11 * dx - j01 * dy) / det
    l2 = (j00 * dy - j10 * dx) / det
    return numpy.stack([1.0 - l1 - l2, l1, l2])


def edge_midpoints(mesh):
    e = mesh.edges
    return 0.5 * (mesh.points[e[:, 0]] + mesh.points[e[:, 1]])


def obstacle_vertices(mesh, box):
    '''Boundary vertices strictly inside the outer box (x0, x1, y0, y1): the
    obstacle's.'''
    x0, x1, y0, y1 = box
    v = numpy.unique(mesh.edges[mesh.bfacets].ravel())
    p = mesh.points[v]
    eps = 1e-12
    inside = (p[:, 0] > x0 + eps) & (p[:, 0] < x1 - eps) \
        & (p[:, 1] > y0 + eps) & (p[:, 1] < y1 - eps)
    return p[inside]


def random_points(mesh, n, seed=0, margin=0.05):
    '''n uniform points in the bounding box widened by `margin` of its size
    on every side (some outside the mesh, some in a hole).'''
    rng = numpy.random.RandomState(seed)
    lo, hi = mesh.points.min(axis=0), mesh.points.max(axis=0)
    ext = hi - lo
    return lo - margin * ext + rng.uniform(size=(n, 2)) * (1 + 2 * margin) * ext
