# -*- coding: utf-8 -*-
'''
Contour lines, their length and the area above them in numpy: an independent
restatement of the definitions of flow_amd/fem/isolines.py, for the tests.

It reads layout.cell_dofs and layout.dof_coords only.  Every sub-triangle is
turned counter-clockwise by its own signed area; walking its three edges in
that order, the segment STARTS on the edge that goes from a node above to a
node below and ENDS on the edge that goes from below to above (the above side
is then on the left).  The area of {f_h >= c} in a sub-triangle is the shoelace
area of the polygon that clipping the triangle against the half plane leaves --
not the product formula of the kernel.
'''
import numpy

from flow_amd import fem

# local nodes of the sub-triangles, [v0 v1 v2 e0 e1 e2], e_i opposite v_i: the
# corner triangles at v0, v1, v2, then the middle one
SUBS = {1: ((0, 1, 2),),
        2: ((0, 5, 4), (1, 3, 5), (2, 4, 3), (3, 4, 5))}


def diameter(mesh):
    '''The diagonal of the mesh's bounding box.'''
    p = mesh.points
    return float(numpy.hypot(*(p.max(axis=0) - p.min(axis=0))))


class Triangulation(object):
    '''The sub-triangles of a scalar P1 / P2 layout: T (nc, ns, 3) global
    dofs, each counter-clockwise; X (N, 2) the dof coordinates.'''

    def __init__(self, layout):
        cd = numpy.asarray(layout.cell_dofs, dtype=numpy.int64)
        self.X = numpy.asarray(layout.dof_coords, dtype=numpy.float64)
        T = numpy.stack([cd[:, list(s)] for s in SUBS[layout.degree]], axis=1)
        P = self.X[T]                                     # (nc, ns, 3, 2)
        d1, d2 = P[:, :, 1] - P[:, :, 0], P[:, :, 2] - P[:, :, 0]
        signed = 0.5 * (d1[..., 0] * d2[..., 1] - d1[..., 1] * d2[..., 0])
        cw = signed < 0.0
        T[cw] = T[cw][:, [0, 2, 1]]
        self.T = T
        self.area = numpy.abs(signed)                     # (nc, ns)
        self.nc, self.ns = T.shape[:2]

    def boundary_keys(self):
        '''The sub-edges (a, b), a < b, that lie in one sub-triangle only.'''
        e = numpy.concatenate([self.T[:, :, [k, (k + 1) % 3]].reshape(-1, 2)
                               for k in range(3)])
        e.sort(axis=1)
        uniq, count = numpy.unique(e, axis=0, return_counts=True)
        assert count.max() <= 2
        return set(map(tuple, uniq[count == 1].tolist()))


def _crossing(X, f, u, v, c):
    a, b = numpy.minimum(u, v), numpy.maximum(u, v)
    t = (c - f[a]) / (f[b] - f[a])
    return a, b, X[a] + t[:, None] * (X[b] - X[a])


def segments(layout, f, levels, tri=None):
    '''dict: xy (nseg, 4), level, cell, sub (nseg,), keys (nseg, 4), ordered
    by cell, then level, then sub-triangle; gap: the smallest |f_b - f_a|
    over the crossed sub-edges (inf where there is none).'''
    tri = tri or Triangulation(layout)
    f = numpy.asarray(f, dtype=numpy.float64)
    levels = numpy.atleast_1d(numpy.asarray(levels, dtype=numpy.float64))
    F = f[tri.T]                                          # (nc, ns, 3)
    finite = numpy.isfinite(F).all(axis=-1)
    rows = {k: [] for k in ('xy', 'level', 'cell', 'sub', 'keys')}
    gap = numpy.inf
    for k, c in enumerate(levels):
        above = F >= c
        na = above.sum(axis=-1)
        # the one node above lies on the level: a point, no segment
        peak = (na == 1) & (above & (F == c)).any(axis=-1)
        cell, sub = numpy.nonzero(finite & (na > 0) & (na < 3) & ~peak)
        if len(cell) == 0:
            continue
        t, ab = tri.T[cell, sub], above[cell, sub]
        nxt = numpy.roll(ab, -1, axis=1)
        kout = numpy.argmax(ab & ~nxt, axis=1)            # above -> below
        kin = numpy.argmax(~ab & nxt, axis=1)             # below -> above
        r = numpy.arange(len(cell))
        a0, b0, p0 = _crossing(tri.X, f, t[r, kout], t[r, (kout + 1) % 3], c)
        a1, b1, p1 = _crossing(tri.X, f, t[r, kin], t[r, (kin + 1) % 3], c)
        gap = min(gap, numpy.abs(f[b0] - f[a0]).min(),
                  numpy.abs(f[b1] - f[a1]).min())
        rows['xy'].append(numpy.concatenate([p0, p1], axis=1))
        rows['keys'].append(numpy.stack([a0, b0, a1, b1], axis=1))
        rows['level'].append(numpy.full(len(cell), k, dtype=numpy.int64))
        rows['cell'].append(cell)
        rows['sub'].append(sub)
    if not rows['cell']:
        return {'xy': numpy.zeros((0, 4)), 'keys': numpy.zeros((0, 4), numpy.int64),
                'level': numpy.zeros(0, numpy.int64), 'gap': gap,
                'cell': numpy.zeros(0, numpy.int64),
                'sub': numpy.zeros(0, numpy.int64)}
    out = {k: numpy.concatenate(v) for k, v in rows.items()}
    order = numpy.lexsort((out['sub'], out['level'], out['cell']))
    out = {k: v[order] for k, v in out.items()}
    out['gap'] = gap
    return out


def length(layout, f, levels, tri=None):
    '''(nlevels,): the summed lengths of the segments of every level.'''
    levels = numpy.atleast_1d(numpy.asarray(levels, dtype=numpy.float64))
    s = segments(layout, f, levels, tri)
    each = numpy.hypot(s['xy'][:, 2] - s['xy'][:, 0], s['xy'][:, 3] - s['xy'][:, 1])
    return numpy.bincount(s['level'], weights=each, minlength=len(levels))


def _clipped_area(P, g):
    '''Area of the part of the triangle P (3, 2) where the linear function
    with nodal values g (3,) is >= 0: clip, then the shoelace formula.'''
    poly = []
    for k in range(3):
        j = (k + 1) % 3
        if g[k] >= 0.0:
            poly.append(P[k])
        if (g[k] >= 0.0) != (g[j] >= 0.0):
            poly.append(P[k] + (g[k] / (g[k] - g[j])) * (P[j] - P[k]))
    if len(poly) < 3:
        return 0.0
    Q = numpy.array(poly)
    x, y = Q[:, 0], Q[:, 1]
    return 0.5 * abs(numpy.dot(x, numpy.roll(y, -1)) - numpy.dot(y, numpy.roll(x, -1)))


def area(layout, f, levels, tri=None):
    '''(nlevels,): the area of {f_h >= c} for every level.'''
    tri = tri or Triangulation(layout)
    f = numpy.asarray(f, dtype=numpy.float64)
    levels = numpy.atleast_1d(numpy.asarray(levels, dtype=numpy.float64))
    F = f[tri.T]
    finite = numpy.isfinite(F).all(axis=-1)
    out = numpy.zeros(len(levels))
    for k, c in enumerate(levels):
        na = (F >= c).sum(axis=-1)
        total = tri.area[finite & (na == 3)].sum()
        for cell, sub in zip(*numpy.nonzero(finite & (na > 0) & (na < 3))):
            t = tri.T[cell, sub]
            total += _clipped_area(tri.X[t], f[t] - c)
        out[k] = total
    return out


# -- what the host and the device tests share ---------------------------------------
# the restatement's ratio of the length errors on the quarter circle (measured:
# tests/test_isolines_host.py has the figures), less 25 %
QUARTER_CIRCLE_MARGIN = 0.75 * 4.8634

A = numpy.array([0.7, -0.4])


def hole_mesh():
    '''rectangle_with_hole at the smallest size at which the hole has an
    interior boundary of its own and the counts are odd.'''
    return fem.rectangle_with_hole(0.0, 1.0, 0.0, 1.0, (0.5, 0.5), 0.2, 9, 7)


def nodal(V, fn):
    xy = V.layout.dof_coords
    return fn(xy[:, 0], xy[:, 1])


def clip_square(a, c):
    '''(chord length, area) of {a . x >= c} in the unit square.'''
    P = numpy.array([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0]])
    g = P @ a - c
    poly, cuts = [], []
    for k in range(4):
        j = (k + 1) % 4
        if g[k] >= 0.0:
            poly.append(P[k])
        if (g[k] >= 0.0) != (g[j] >= 0.0):
            x = P[k] + g[k] / (g[k] - g[j]) * (P[j] - P[k])
            poly.append(x)
            cuts.append(x)
    Q = numpy.array(poly)
    area = 0.5 * abs(numpy.dot(Q[:, 0], numpy.roll(Q[:, 1], -1))
                     - numpy.dot(Q[:, 1], numpy.roll(Q[:, 0], -1)))
    return float(numpy.hypot(*(cuts[0] - cuts[1]))), area


def quarter_circle_errors(length_of):
    '''|length - 0.3 pi| of the contour x^2 + y^2 = 0.36 of the P2 nodal
    values on UnitSquareMesh(8, 8) and (16, 16); length_of(V, f_values, c).'''
    errs = []
    for n in (8, 16):
        V = fem.FunctionSpace(fem.UnitSquareMesh(n, n), 'CG', 2)
        f = nodal(V, lambda x, y: x * x + y * y)
        errs.append(abs(length_of(V, f, 0.36) - 0.3 * numpy.pi))
    return errs
