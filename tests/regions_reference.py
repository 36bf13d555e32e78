# -*- coding: utf-8 -*-
'''
Connected components of a level set and their measures in numpy and scipy: an
independent restatement of the definitions of flow_amd/fem/regions.py, for
the tests.

It reads layout.cell_dofs and layout.dof_coords and the mesh's vertices only.
Components come from scipy.sparse.csgraph.connected_components on the graph of
the sub-edges with two inside dofs, relabelled by smallest dof.  A piece is
the polygon that walking the sub-triangle's edges leaves (inside nodes and
crossings), with the definition's diagonal; g is evaluated at a PHYSICAL point
through the barycentric coordinates of the parent cell computed from its
vertices -- not interpolated along the sub-edges as the kernel does.
'''
import numpy
import scipy.sparse
import scipy.sparse.csgraph

from isolines_reference import Triangulation, hole_mesh, nodal   # noqa: F401


def inside(f, level, side='above'):
    f = numpy.asarray(f, dtype=numpy.float64)
    with numpy.errstate(invalid='ignore'):
        return numpy.isfinite(f) & ((f >= level) if side == 'above' else (f < level))


def sub_edges(tri):
    '''(m, 2) the sub-edges of the triangulation, each once per sub-triangle.'''
    return numpy.concatenate([tri.T[:, :, [k, (k + 1) % 3]].reshape(-1, 2)
                              for k in range(3)])


def components(tri, ins):
    '''(labels (N,): the smallest dof of the component, -1 outside;
    graph: the csr matrix of the inside sub-edges).'''
    N = len(tri.X)
    e = sub_edges(tri)
    e = e[ins[e[:, 0]] & ins[e[:, 1]]]
    graph = scipy.sparse.coo_matrix(
        (numpy.ones(len(e)), (e[:, 0], e[:, 1])), shape=(N, N)).tocsr()
    _, comp = scipy.sparse.csgraph.connected_components(graph, directed=False)
    smallest = numpy.full(comp.max() + 1, N, dtype=numpy.int64)
    numpy.minimum.at(smallest, comp, numpy.arange(N))
    labels = numpy.where(ins, smallest[comp], -1)
    return labels, graph


def diameter(tri, ins):
    '''The largest graph distance (in sub-edges) between two inside dofs of
    one component: the sweeps a plain neighbour-minimum may need.'''
    _, graph = components(tri, ins)
    d = scipy.sparse.csgraph.shortest_path(graph, unweighted=True, directed=False)
    return int(d[numpy.isfinite(d)].max())


def _basis(deg, lam):
    if deg == 1:
        return lam
    l0, l1, l2 = lam
    return numpy.array([l0 * (2 * l0 - 1), l1 * (2 * l1 - 1), l2 * (2 * l2 - 1),
                        4 * l1 * l2, 4 * l0 * l2, 4 * l0 * l1])


def _triangle(P, cell_xy, gdeg, G):
    '''Integrals of 1, x, y and the rows of G (ncomp, nloc) over the triangle
    P (3, 2) by the edge-midpoint rule.'''
    d1, d2 = P[1] - P[0], P[2] - P[0]
    area = 0.5 * abs(d1[0] * d2[1] - d1[1] * d2[0])
    out = numpy.zeros(3 + len(G))
    out[0] = area
    M = numpy.array([cell_xy[1] - cell_xy[0], cell_xy[2] - cell_xy[0]]).T
    for k in range(3):
        m = 0.5 * (P[k] + P[(k + 1) % 3])
        out[1:3] += area / 3.0 * m
        if len(G):
            s, t = numpy.linalg.solve(M, m - cell_xy[0])
            out[3:] += area / 3.0 * (G @ _basis(gdeg, numpy.array([1.0 - s - t, s, t])))
    return out


def _crossing(X, f, u, v, c):
    a, b = min(u, v), max(u, v)
    t = (c - f[a]) / (f[b] - f[a])
    return X[a] + t * (X[b] - X[a])


def regions(layout, f, level, side='above', g=None, glayout=None, tri=None):
    '''dict: count; labels (N,) compact ids, -1 outside; root, size (count,);
    moments (3 + ncomp, count): the integrals of 1, x, y, g_a; scale, the
    same shape: the sums of |triangle integrals|; area, centroid; and, where g
    has the degree of the layout, gmin, gmax (ncomp, count) over the dofs.
    g: (ncomp, glayout.N) nodal values on the same mesh.'''
    tri = tri or Triangulation(layout)
    f = numpy.asarray(f, dtype=numpy.float64)
    ins = inside(f, level, side)
    small, _ = components(tri, ins)
    root = numpy.unique(small[small >= 0])
    count = len(root)
    labels = numpy.where(small >= 0, numpy.searchsorted(root, small), -1)
    size = numpy.bincount(labels[labels >= 0], minlength=count)
    if g is None:
        G_all, gdeg = numpy.zeros((0, 0)), 1
    else:
        G_all = numpy.atleast_2d(numpy.asarray(g, dtype=numpy.float64))
        gdeg = glayout.degree
    nrows = 3 + len(G_all)
    moments, scale = numpy.zeros((nrows, count)), numpy.zeros((nrows, count))
    mesh = layout.mesh
    for c in range(tri.nc):
        cell_xy = mesh.points[mesh.cell_vertices[c]]
        G = G_all[:, glayout.cell_dofs[c]] if len(G_all) else numpy.zeros((0, 0))
        for s in range(tri.ns):
            t = tri.T[c, s]
            if not numpy.isfinite(f[t]).all() or not ins[t].any():
                continue
            k_in = numpy.nonzero(ins[t])[0]
            owner = labels[t[k_in[0]]]
            assert (labels[t[k_in]] == owner).all()
            if len(k_in) == 3:
                tris = [tri.X[t]]
            elif len(k_in) == 1:
                p = k_in[0]
                q, r = t[(p + 1) % 3], t[(p + 2) % 3]
                tris = [numpy.array([tri.X[t[p]],
                                     _crossing(tri.X, f, t[p], q, level),
                                     _crossing(tri.X, f, t[p], r, level)])]
            else:
                p = numpy.nonzero(~ins[t])[0][0]           # C, the node outside
                a, b = t[(p + 1) % 3], t[(p + 2) % 3]
                P = _crossing(tri.X, f, a, t[p], level)
                Q = _crossing(tri.X, f, b, t[p], level)
                tris = [numpy.array([tri.X[a], tri.X[b], Q]),
                        numpy.array([tri.X[a], Q, P])]
            for T in tris:
                v = _triangle(T, cell_xy, gdeg, G)
                moments[:, owner] += v
                scale[:, owner] += numpy.abs(v)
    out = {'count': count, 'labels': labels, 'root': root, 'size': size,
           'moments': moments, 'scale': scale, 'area': moments[0].copy()}
    with numpy.errstate(invalid='ignore', divide='ignore'):
        out['centroid'] = (moments[1:3] / moments[0:1]).T
    if g is not None and glayout.degree == layout.degree:
        out['gmin'] = numpy.array([[row[labels == k].min() for k in range(count)]
                                   for row in G_all]).reshape(len(G_all), count)
        out['gmax'] = numpy.array([[row[labels == k].max() for k in range(count)]
                                   for row in G_all]).reshape(len(G_all), count)
    return out


def polygon_area(P):
    x, y = P[:, 0], P[:, 1]
    return 0.5 * abs(numpy.dot(x, numpy.roll(y, -1)) - numpy.dot(y, numpy.roll(x, -1)))
