# -*- coding: utf-8 -*-
'''
Numpy restatement of fem.BoundaryProfile (helper, not a test): the boundary
curves chained from `mesh.bfacets`, the sample coordinates, arclengths,
weights and normals, and an evaluator of P1 / P2 fields, their gradients and
Expression lattices on the owning cell at the samples, written from the basis
tables of fem/reference.py.  It never calls flow_amd/fem/profile.py.

Orientation here comes from the signed area of the owning cell (the edge a->b
has the cell on its left iff cross(b - a, c - a) > 0, c the cell's third
vertex), not from the normal; samples are laid along the traversal directly
(head + s (tail - head), s ascending), not through the kernel's rule rows.
'''
import numpy

from flow_amd.fem import reference
from flow_amd.fem.function import cell_lattice_points


def _oriented(mesh, pos):
    '''(head, tail) vertex ids of the boundary facets at positions pos of
    mesh.bfacets, the domain on the left.'''
    P = mesh.points
    out = []
    for k in pos:
        a, b = (int(v) for v in mesh.edges[mesh.bfacets[k]])
        cv = [int(v) for v in mesh.cell_vertices[mesh.bfacet_cell[k]]]
        c, = [v for v in cv if v not in (a, b)]
        ab, ac = P[b] - P[a], P[c] - P[a]
        left = ab[0] * ac[1] - ab[1] * ac[0] > 0.0
        out.append((a, b) if left else (b, a))
    return out


def chain(mesh, pos, start=None):
    '''[(list of positions in mesh.bfacets, closed)] in the order of the
    specification: domain on the left, closed curves from their
    lexicographically smallest vertex (or the vertex nearest `start`), open
    ones from the end without a predecessor, curves sorted by first vertex.'''
    P = mesh.points
    pos = [int(k) for k in pos]
    ends = dict(zip(pos, _oriented(mesh, pos)))
    by_head = {}
    tails = set()
    for k in pos:
        assert ends[k][0] not in by_head
        by_head[ends[k][0]] = k
        tails.add(ends[k][1])
    key = lambda v: (P[v][0], P[v][1])
    near = None
    if start is not None:
        verts = sorted(set(by_head) | tails, key=key)
        near = min(verts, key=lambda v: numpy.hypot(P[v][0] - start[0],
                                                     P[v][1] - start[1]))
    left = set(pos)
    curves = []
    for k in pos:
        if ends[k][0] in tails:
            continue
        walk = []
        while k is not None:
            walk.append(k)
            left.discard(k)
            k = by_head.get(ends[k][1])
        curves.append((walk, False))
    while left:
        k = k0 = min(left)
        walk = []
        while True:
            walk.append(k)
            left.discard(k)
            k = by_head[ends[k][1]]
            if k == k0:
                break
        heads = [ends[j][0] for j in walk]
        first = heads.index(near) if near in heads \
            else heads.index(min(heads, key=key))
        curves.append((walk[first:] + walk[:first], True))
    curves.sort(key=lambda c: key(ends[c[0][0]][0]))
    return curves, ends


class Reference(object):
    def __init__(self, mesh, pos, degree, start=None):
        self.mesh = mesh
        P = mesh.points
        curves, ends = chain(mesh, pos, start)
        self.curves = curves
        x, w = numpy.polynomial.legendre.leggauss(degree // 2 + 1)
        t, w = 0.5 * (x + 1.0), 0.5 * w
        self.m = m = len(t)
        X, S, W, N, C, LEN, offs = [], [], [], [], [], [], [0]
        for walk, _ in curves:
            run = 0.0
            for k in walk:
                h, tl = P[ends[k][0]], P[ends[k][1]]
                d = tl - h
                L = float(numpy.hypot(d[0], d[1]))
                X.append(h[None, :] + t[:, None] * d[None, :])
                S.append(run + t * L)
                W.append(w * L)
                # domain on the left: the outward normal is to the right
                N.append(numpy.repeat([[d[1] / L, -d[0] / L]], m, axis=0))
                C.append(numpy.full(m, mesh.bfacet_cell[k]))
                LEN.append(L)
                run += L
            offs.append(offs[-1] + len(walk))
        self.offsets = numpy.array(offs)
        self.order = numpy.array([k for walk, _ in curves for k in walk],
                                 dtype=numpy.int64)
        self.closed = numpy.array([c for _, c in curves], dtype=bool)
        self.length = numpy.array(LEN)
        n = len(self.order) * m
        self.x = numpy.concatenate(X).T if n else numpy.zeros((2, 0))
        self.s = numpy.concatenate(S) if n else numpy.zeros(0)
        self.weights = numpy.concatenate(W) if n else numpy.zeros(0)
        self.normal = numpy.concatenate(N).T if n else numpy.zeros((2, 0))
        self.cells = numpy.concatenate(C).astype(numpy.int64) if n \
            else numpy.zeros(0, dtype=numpy.int64)
        V = P[mesh.cell_vertices[self.cells]]                   # (n, 3, 2)
        J = numpy.stack([V[:, 1] - V[:, 0], V[:, 2] - V[:, 0]], axis=2)
        self.Jinv = numpy.linalg.inv(J) if n else numpy.zeros((0, 2, 2))
        self.ref = numpy.einsum('nrd,nd->nr', self.Jinv, self.x.T - V[:, 0])
        self.V = V

    def _dofs(self, f, comp):
        W = f.function_space()
        U = f.array().reshape(W.dim, W.N)[comp]
        return W.degree, U[W.layout.cell_dofs[self.cells]]       # (n, nloc)

    def field(self, f, comp=0):
        deg, U = self._dofs(f, comp)
        return numpy.einsum('nj,nj->n', U, reference.tabulate(deg, self.ref))

    def grad(self, f, comp=0):
        '''(2, n): d/dx and d/dy on the owning cell.'''
        deg, U = self._dofs(f, comp)
        g = numpy.einsum('nj,njr->nr', U, reference.tabulate_grad(deg, self.ref))
        return numpy.einsum('nrd,nr->dn', self.Jinv, g)

    def expression(self, e, comp=0):
        k = int(e.degree)
        X = cell_lattice_points(self.mesh, k)
        nc, nl = X.shape[:2]
        lat = e.eval(X.reshape(-1, 2).T).reshape(-1, nc, nl)[comp][self.cells]
        return numpy.einsum('nl,nl->n', lat, reference.tabulate(k, self.ref))

    def diameter(self):
        V = self.V
        d = [numpy.hypot(*(V[:, i] - V[:, j]).T) for i, j in ((0, 1), (1, 2), (2, 0))]
        return numpy.maximum(d[0], numpy.maximum(d[1], d[2]))

    def facet_sums(self, values):
        '''Per-facet integrals of sample values (..., n) -> (..., nfacets).'''
        v = values * self.weights
        return v.reshape(v.shape[:-1] + (-1, self.m)).sum(axis=-1)
