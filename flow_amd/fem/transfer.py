# -*- coding: utf-8 -*-
'''
Fields from one space or mesh to another: dolfin's `interpolate(u, V)` and
`w.interpolate(u)` for a discrete u, as an object that is set up once,

    T = Transfer(V_from, V_to)
    T.apply(u_from, out=w)          # every time step, no host synchronisation

between scalar or 2-vector P1 / P2 spaces of the same number of components.
Every target node (V_to.layout.dof_coords) gets a cell of the source mesh and
barycentric coordinates there, once; apply() evaluates the source field at
them (flow_transfer_apply, csrc/transfer_kernels.hip: one lane per node, the
P1 / P2 basis straight-line, all components in one launch).

Same mesh: no location.  A node's cell is the lowest-index cell that holds it
and its coordinates are the reference lattice's exact 0, 1/2 and 1, taken from
the target layout's cell_dofs: P1 -> P1 and P2 -> P2 copy, P2 -> P1 takes the
vertex values, P1 -> P2 the vertex values and the edge means.

Other mesh: flow_locate_points (the lowest-index rule of flow_amd/fem/
points.py).  Two meshes of one domain approximate a curved boundary by
different polygons, so some target nodes lie in no source cell.  Without
allow_extrapolation that is a ValueError.  With it such a node takes the
NEAREST POINT OF THE SOURCE MESH (flow_nearest_cells): the boundary facet of
smallest squared distance, ties to the lowest facet index (the order of
mesh.bfacets), its owning cell, and the barycentric coordinates of the foot
point clamped to the facet.  This is a clamp, NOT dolfin's polynomial
extrapolation: the node gets a value the source field takes on that boundary
edge, so it stays within the range of the edge's values (for P2: of the
quadratic along the edge), where the cell's polynomial continued outward does
not.  `distance` tells how far each node was moved; max_distance bounds it.

Not on strips.
'''
import numpy

from .points import BOX_PAD, PointGrid, _grid_struct

# boundary facets per bucket of the facet grid aimed at: the boundary is a
# curve, so most buckets are empty and those on it hold about sqrt(16) times
# fewer facets than with one bucket per facet
FACET_BUCKETS = 16.0


def _scalar_or_vector(V, what):
    '''The refusals of Transfer for one space.'''
    if not hasattr(V, 'layout'):
        raise NotImplementedError(
            '%s: a mixed space; transfer its sub-spaces one by one' % what)
    if getattr(V, 'component', None) is not None:
        raise NotImplementedError(
            '%s: a component view (W.sub(i)); transfer the vector field, or '
            'a Function on W.sub(i).collapse()' % what)
    if V.degree not in (1, 2) or V.dim not in (1, 2):
        raise NotImplementedError('%s: P%r with %r components; scalar or '
                                  '2-vector P1 / P2' % (what, V.degree, V.dim))


def same_mesh_table(lay_from, lay_to):
    '''(cells (N_to,) int32, bary (3, N_to)) of the nodes of lay_to on their
    own mesh, host only: the lowest-index cell that has the node among its
    dofs and the node's place on the reference lattice (vertex i: e_i; the
    edge opposite vertex i: 1/2 at the other two).  lay_from only has to
    live on the same mesh: the table does not depend on its degree.'''
    assert lay_from.mesh is lay_to.mesh
    nloc = lay_to.nloc
    flat = lay_to.cell_dofs.ravel()                     # cell-major
    order = numpy.argsort(flat, kind='stable')
    first = numpy.zeros(lay_to.N + 1, dtype=numpy.int64)
    numpy.cumsum(numpy.bincount(flat, minlength=lay_to.N), out=first[1:])
    assert (numpy.diff(first) > 0).all(), 'a dof in no cell'
    at = order[first[:-1]]                              # first = lowest cell
    lattice = numpy.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0],
                           [0.0, 0.5, 0.5], [0.5, 0.0, 0.5], [0.5, 0.5, 0.0]])
    cells = (at // nloc).astype(numpy.int32)
    bary = numpy.ascontiguousarray(lattice[at % nloc].T)
    return cells, bary


class FacetGrid(PointGrid):
    '''The bucket grid of a mesh's boundary facets (layout of flow_point_grid,
    host arrays): `cells` holds indices into mesh.bfacets / bfacet_cell /
    bfacet_local, every facet in each bucket its padded bounding box
    overlaps, ascending within a bucket.'''

    def __init__(self, mesh, buckets_per_facet=FACET_BUCKETS):
        p = mesh.points
        seg = p[mesh.edges[mesh.bfacets]]               # (nf, 2, 2)
        nf = len(seg)
        lo, hi = p.min(axis=0), p.max(axis=0)
        ext = numpy.maximum(hi - lo, 1e-300)
        nb = max(1.0, nf * float(buckets_per_facet))
        nx = int(max(1, min(nb, round(numpy.sqrt(nb * ext[0] / ext[1])))))
        ny = int(max(1, round(nb / nx)))
        self.nx, self.ny = nx, ny
        self.x0, self.y0 = float(lo[0]), float(lo[1])
        self.hx_inv = float(nx / ext[0])
        self.hy_inv = float(ny / ext[1])
        blo, bhi = seg.min(axis=1), seg.max(axis=1)
        pad = BOX_PAD * (bhi - blo).sum(axis=1)
        blo = blo - pad[:, None]
        bhi = bhi + pad[:, None]
        i0, j0 = self.bucket_xy(blo)
        i1, j1 = self.bucket_xy(bhi)
        w = (i1 - i0 + 1).astype(numpy.int64)
        count = w * (j1 - j0 + 1)
        facet = numpy.repeat(numpy.arange(nf, dtype=numpy.int64), count)
        first = numpy.cumsum(count) - count
        k = numpy.arange(len(facet), dtype=numpy.int64) - first[facet]
        bucket = (j0[facet] + k // w[facet]) * nx + i0[facet] + k % w[facet]
        order = numpy.argsort(bucket, kind='stable')
        self.cells = facet[order].astype(numpy.int32)
        start = numpy.zeros(nx * ny + 1, dtype=numpy.int64)
        numpy.cumsum(numpy.bincount(bucket, minlength=nx * ny), out=start[1:])
        assert start[-1] < 2**31
        self.start = start.astype(numpy.int32)

    def ring(self, pt, r):
        '''The buckets of ring r around the (clamped) bucket of the point:
        those at Chebyshev distance r that lie in the grid.'''
        ix, iy = self.bucket_xy(numpy.asarray(pt, dtype=float).reshape(1, 2))
        ix, iy = int(ix[0]), int(iy[0])
        out = []
        for j in range(max(iy - r, 0), min(iy + r, self.ny - 1) + 1):
            for i in range(max(ix - r, 0), min(ix + r, self.nx - 1) + 1):
                if max(abs(i - ix), abs(j - iy)) == r:
                    out.append(j * self.nx + i)
        return out

    def ring_bound(self, pt, r):
        '''No point of a bucket beyond ring r is nearer to the point than
        this (inf: there are no such buckets): the kernel's stopping rule
        (csrc/transfer_kernels.hip), its slack included.'''
        tx = (float(pt[0]) - self.x0) * self.hx_inv
        ty = (float(pt[1]) - self.y0) * self.hy_inv
        ix, iy = self.bucket_xy(numpy.asarray(pt, dtype=float).reshape(1, 2))
        ix, iy = int(ix[0]), int(iy[0])
        wx, wy = 1.0 / self.hx_inv, 1.0 / self.hy_inv
        bound = numpy.inf
        if ix - r > 0:
            bound = min(bound, (tx - (ix - r)) * wx)
        if ix + r < self.nx - 1:
            bound = min(bound, (ix + r + 1 - tx) * wx)
        if iy - r > 0:
            bound = min(bound, (ty - (iy - r)) * wy)
        if iy + r < self.ny - 1:
            bound = min(bound, (iy + r + 1 - ty) * wy)
        return bound - 1.0e-9 * (wx + wy)

    def search(self, pt, distance2):
        '''The facets a lane looks at for the point, ring by ring, as the
        kernel does: distance2(facets) -> their squared distances.  Returns
        the list of candidate facets (with repeats removed).'''
        seen, best = [], numpy.inf
        for r in range(max(self.nx, self.ny)):
            for b in self.ring(pt, r):
                cand = self.candidates(b)
                if len(cand):
                    seen.append(cand)
                    best = min(best, float(distance2(cand).min()))
            bound = self.ring_bound(pt, r)
            if bound == numpy.inf or (bound > 0.0 and bound * bound > best):
                break
        return numpy.unique(numpy.concatenate(seen)) if seen \
            else numpy.zeros(0, dtype=numpy.int32)


def facet_grid(mesh):
    '''The mesh's facet grid, built once.'''
    held = mesh._cache.get('facet_grid')
    if held is None:
        held = mesh._cache['facet_grid'] = FacetGrid(mesh)
    return held


def _facet_grid_struct(mesh):
    '''(flow_point_grid of the facets, facet_cell, facet_local, nfacets),
    uploaded once per device.'''
    from .. import _hip, device
    cache = mesh._cache.setdefault('facet_grid_dev', {})
    key = str(device.get())
    held = cache.get(key)
    if held is None:
        g = facet_grid(mesh)
        start, cells = device.to_device(g.start), device.to_device(g.cells)
        fc = device.to_device(mesh.bfacet_cell.astype(numpy.int32))
        fl = device.to_device(mesh.bfacet_local.astype(numpy.int32))
        s = _hip.PointGridS(
            g.nx, g.ny, g.x0, g.y0, g.hx_inv, g.hy_inv,
            _hip.i32(start, len(g.start), 'facet grid start'),
            _hip.i32(cells, len(g.cells), 'facet grid facets'))
        held = cache[key] = (s, fc, fl, len(mesh.bfacets), start, cells)
    return held[:4]


class Transfer(object):
    '''Interpolation of Functions of V_from into V_to, located once.

        T = Transfer(V_from, V_to, allow_extrapolation=False, max_distance=None)
        w = T.apply(u)              # a Function on V_to
        T.apply(u, out=w)           # into w; enqueued, no host synchronisation
        T.cells, T.found, T.distance

    Per target node (host arrays): `cells` the source cell (int32), `found`
    whether the node lies in the source mesh, `distance` how far it is from
    it (0 where found).  A node outside takes the nearest point of the source
    mesh, on a boundary facet: a clamp, not dolfin's polynomial
    extrapolation (see the module's docstring); without allow_extrapolation,
    or farther than max_distance, it is a ValueError.'''

    def __init__(self, V_from, V_to, allow_extrapolation=False,
                 max_distance=None):
        import ctypes
        import torch
        from .. import _hip, device
        from .ops import _no_strips, mesh_struct
        _scalar_or_vector(V_from, 'V_from')
        _scalar_or_vector(V_to, 'V_to')
        if V_from.dim != V_to.dim:
            raise ValueError('V_from has %d component(s), V_to %d'
                             % (V_from.dim, V_to.dim))
        _no_strips('Field transfer')
        self.V_from, self.V_to = V_from, V_to
        lay = V_to.layout
        n = self.n = lay.N
        if V_from.mesh() is V_to.mesh():
            cells, bary = same_mesh_table(V_from.layout, lay)
            self._cell = device.to_device(cells)
            self._bary = device.to_device(bary.reshape(-1))
            self.cells = cells
            self.found = numpy.ones(n, dtype=bool)
            self.distance = numpy.zeros(n)
            return
        mesh = V_from.mesh()
        pts = lay.dof_coords
        xy = device.to_device(pts.T.copy())
        self._cell = torch.empty(n, dtype=torch.int32, device=xy.device)
        self._bary = device.empty(3 * n)
        _hip.check(_hip.lib().flow_locate_points(
            ctypes.byref(mesh_struct(mesh)), ctypes.byref(_grid_struct(mesh)),
            n, _hip.f64(xy, 2 * n, 'points'), _hip.i32(self._cell, n, 'cells'),
            _hip.f64(self._bary, 3 * n, 'barycentric coordinates'),
            _hip.stream()))
        self.found = device.to_host(self._cell).numpy()[:n] >= 0
        self.distance = numpy.zeros(n)
        if not self.found.all():
            if not allow_extrapolation:
                self._refuse(~self.found, pts, 'lie in no cell of the source '
                             'mesh (allow_extrapolation=True gives them the '
                             'nearest point of it)')
            gs, fc, fl, nf = _facet_grid_struct(mesh)
            dist = device.empty(n)
            _hip.check(_hip.lib().flow_nearest_cells(
                ctypes.byref(mesh_struct(mesh)), ctypes.byref(gs), nf,
                _hip.i32(fc, nf, 'facet cells'), _hip.i32(fl, nf, 'facet locals'),
                n, _hip.f64(xy, 2 * n, 'points'),
                _hip.i32(self._cell, n, 'cells'),
                _hip.f64(self._bary, 3 * n, 'barycentric coordinates'),
                _hip.f64(dist, n, 'distances'), _hip.stream()))
            self.distance = device.to_host(dist).numpy()[:n].copy()
        self.cells = device.to_host(self._cell).numpy()[:n].copy()
        assert (self.cells >= 0).all()
        if max_distance is not None:
            far = ~(self.distance <= float(max_distance))
            if far.any():
                self._refuse(far, pts, 'are farther than max_distance = %r '
                             'from the source mesh (the farthest: %r)'
                             % (float(max_distance), float(self.distance.max())))

    @staticmethod
    def _refuse(mask, pts, what):
        first = pts[numpy.nonzero(mask)[0][0]]
        raise ValueError('%d of %d target nodes %s; the first: (%r, %r)'
                         % (int(mask.sum()), len(mask), what, float(first[0]),
                            float(first[1])))

    def apply(self, u_from, out=None):
        '''u_from (a Function on V_from) interpolated into V_to: a new
        Function, or `out` (a Function on V_to).  One kernel launch on the
        package's stream, no host synchronisation.'''
        import ctypes
        from .. import _hip, device
        from .function import Function
        from .ops import _no_strips, space_struct
        _no_strips('Field transfer')
        if not isinstance(u_from, Function) \
                or not u_from.function_space().same_as(self.V_from):
            raise ValueError('u_from: not a Function of the space this '
                             'Transfer reads (V_from)')
        if out is None:
            out = Function(self.V_to, device.empty(self.V_to.size()))
        elif not isinstance(out, Function) \
                or not out.function_space().same_as(self.V_to):
            raise ValueError('out: not a Function of the space this Transfer '
                             'writes (V_to)')
        if out.data.data_ptr() == u_from.data.data_ptr():
            raise ValueError('out: the source field itself')
        n, dim = self.n, self.V_to.dim
        _hip.check(_hip.lib().flow_transfer_apply(
            ctypes.byref(space_struct(self.V_from.layout)), dim, n,
            _hip.i32(self._cell, n, 'cells'),
            _hip.f64(self._bary, 3 * n, 'barycentric coordinates'),
            _hip.f64(u_from.data, dim * self.V_from.N, 'u_from'),
            _hip.f64(out.data, dim * n, 'out'), _hip.stream()))
        return out


def interpolate_function(u, V, out=None, allow_extrapolation=False):
    '''fem.interpolate(u, V) and Function.interpolate(u) for a Function u:
    Transfer(u.function_space(), V).apply(u).  The Transfer of a pair of
    spaces on one mesh is a table look-up and kept on the mesh; across meshes
    it locates every node, so hold a Transfer where it is used repeatedly.'''
    V_from = u.function_space()
    if V_from.mesh() is V.mesh() and hasattr(V, 'layout') \
            and getattr(V, 'component', None) is None:
        from .. import device
        key = ('transfer', V_from.degree, V.degree, V_from.dim, V.dim,
               str(device.get()))
        T = V.mesh()._cache.get(key)
        if T is None:
            T = V.mesh()._cache[key] = Transfer(V_from, V)
    else:
        T = Transfer(V_from, V, allow_extrapolation=allow_extrapolation)
    return T.apply(u, out=out)
