# -*- coding: utf-8 -*-
'''
Host restatement of flow_amd/fem/distance.py in numpy: the same Jacobi
iteration and the same Hopf-Lax update as csrc/distance_kernels.hip, written
with the same expression tree (every operation rounds once; the kernel keeps
contraction off), independent of the kernels and of the space's contribution
map: the triangles come from `cell_dofs`, the node positions from the cells'
vertex coordinates.

    graph    the P1 triangulation of the dofs: the cells (P1), or every cell
             cut into (v0, e2, e1), (v1, e0, e2), (v2, e1, e0), (e0, e1, e2)
             (P2; local dofs [v0 v1 v2 e0 e1 e2], e_i opposite v_i, the mid
             point of the straight edge)
    update   of C from the triangle (C, A, B): min over the edge A-B of
             T(x) + |C - x| with T linear on the edge
    sweep    new[i] = min(old[i], min over the triangles at i), from 0 at the
             sources and +inf elsewhere, until a sweep changes nothing

`sweeps` counts every sweep run, the last one -- which changed nothing --
included.
'''
import numpy

# the sub-triangles of a cell by local dof index
SUB = {1: numpy.array([[0, 1, 2]]),
       2: numpy.array([[0, 5, 4], [1, 3, 5], [2, 4, 3], [3, 4, 5]])}


def cell_nodes(degree, cell_points):
    '''Positions (nc, nloc, 2) of the local nodes from the cells' vertex
    coordinates (nc, 3, 2).'''
    P = numpy.asarray(cell_points, dtype=float)
    if degree == 1:
        return P
    mid = numpy.stack([0.5 * (P[:, 1] + P[:, 2]), 0.5 * (P[:, 0] + P[:, 2]),
                       0.5 * (P[:, 0] + P[:, 1])], axis=1)
    return numpy.concatenate([P, mid], axis=1)


class Graph(object):
    '''Every (C, A, B): each sub-triangle of every cell seen from each of its
    three corners, with the geometry that does not change between sweeps.'''

    def __init__(self, degree, cell_dofs, cell_points):
        cd = numpy.asarray(cell_dofs, dtype=numpy.int64)
        X = cell_nodes(degree, cell_points)
        sub = SUB[degree]
        tri = numpy.concatenate([sub[:, [0, 1, 2]], sub[:, [1, 2, 0]],
                                 sub[:, [2, 0, 1]]])             # (3 nsub, 3)
        self.C, self.A, self.B = (cd[:, tri[:, k]].ravel() for k in range(3))
        c, a, b = (X[:, tri[:, k]].reshape(-1, 2) for k in range(3))
        ex, ey = a[:, 0] - b[:, 0], a[:, 1] - b[:, 1]
        px, py = c[:, 0] - b[:, 0], c[:, 1] - b[:, 1]
        qx, qy = c[:, 0] - a[:, 0], c[:, 1] - a[:, 1]
        self.dA = numpy.sqrt(qx * qx + qy * qy)
        self.dB = numpy.sqrt(px * px + py * py)
        self.ee = ex * ex + ey * ey
        self.le = numpy.sqrt(self.ee)
        self.s = (ex * px + ey * py) / self.ee
        self.h = numpy.abs(ex * py - ey * px) / self.le
        # the edges of the (sub-)triangulation: (i, j, |x_i - x_j|), each once
        # per triangle that has it
        self.edges = (self.C, self.A, self.dA)

    def sweep(self, old):
        '''One Jacobi sweep: the new values.'''
        inf = numpy.inf
        ta, tb = old[self.A], old[self.B]
        fa, fb = ta < inf, tb < inf
        best = numpy.full(len(ta), inf)
        # an infinite input is skipped: it is replaced before it is used
        za, zb = numpy.where(fa, ta, 0.0), numpy.where(fb, tb, 0.0)
        best = numpy.where(fa, numpy.minimum(best, za + self.dA), best)
        best = numpy.where(fb, numpy.minimum(best, zb + self.dB), best)
        d = za - zb
        inner = fa & fb & (numpy.abs(d) < self.le)
        with numpy.errstate(invalid='ignore', divide='ignore'):
            t = self.h * d / numpy.sqrt(self.ee - d * d)
            lam = self.s - t / self.le
            inner &= (lam >= 0.0) & (lam <= 1.0)
            c = zb + lam * d + numpy.sqrt(t * t + self.h * self.h)
        best = numpy.where(inner & (c < best), c, best)
        new = old.copy()
        numpy.minimum.at(new, self.C, best)
        return new


def solve(degree, cell_dofs, cell_points, N, sources, max_sweeps=None):
    '''(d (N,), sweeps): the greatest fixed point from 0 at `sources` (dof
    indices or a bool mask) and +inf elsewhere.'''
    g = Graph(degree, cell_dofs, cell_points)
    d = numpy.full(N, numpy.inf)
    d[sources] = 0.0
    limit = N + 1 if max_sweeps is None else max_sweeps
    sweeps = 0
    while True:
        new = g.sweep(d)
        sweeps += 1
        if numpy.array_equal(new, d):
            return d, sweeps
        d = new
        assert sweeps <= limit, 'no dof changes more often than N times'


def distance(V, sources):
    '''solve() on the scalar P1 / P2 space V.'''
    mesh = V.mesh()
    return solve(V.degree, V.layout.cell_dofs, mesh.points[mesh.cell_vertices],
                 V.N, sources)


def lipschitz_excess(V, d):
    '''max over the edges (i, j) of the (sub-)triangulation with finite
    values of |d_i - d_j| / |x_i - x_j|.'''
    mesh = V.mesh()
    i, j, length = Graph(V.degree, V.layout.cell_dofs,
                         mesh.points[mesh.cell_vertices]).edges
    both = numpy.isfinite(d[i]) & numpy.isfinite(d[j])
    return float((numpy.abs(d[i] - d[j])[both] / length[both]).max())


def facet_dofs(V, facets):
    '''The dofs of V on the facets (edge ids): their vertices and, for P2,
    their mid points; sorted.'''
    mesh, layout = V.mesh(), V.layout
    dofs = [layout.vertex_dofs[mesh.edges[facets].ravel()]]
    if V.degree == 2:
        dofs.append(layout.edge_dofs[facets])
    return numpy.unique(numpy.concatenate(dofs))


def diameter(mesh):
    '''The diagonal of the mesh's bounding box.'''
    p = mesh.points
    return float(numpy.hypot(*(p.max(axis=0) - p.min(axis=0))))
