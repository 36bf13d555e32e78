# -*- coding: utf-8 -*-
'''
Fields at points: dolfin's `u(x, y)` / `u(Point(x, y))` and probes -- the
value of a Function, or of any rank <= 1 expression of Functions, Constants
and SpatialCoordinate (flow_amd/fem/forms.py), at given points of the mesh.

Location (flow_locate_points, csrc/form_kernels.hip): point p belongs to the
LOWEST-index cell c with min_k lambda_k^c(p) >= -1e-12 (barycentric
coordinates), or to no cell.  A uniform bucket grid over the mesh's bounding
box (about one bucket per cell, built here with numpy once per mesh, cached
on it and uploaded once) lists, per bucket, every cell whose bounding box --
padded: padding only adds candidates -- overlaps it, in ascending cell
index; a lane tests its bucket's candidates in that order and stops at the
first hit, so the grid never changes the answer.  Points on shared edges
and vertices get one well-defined cell, and a point's cell does not depend
on the other points of the call.

Evaluation (flow_form_points): the form interpreter of the integrals, run
once per point at its stored barycentric coordinates; NaN outside the mesh.
Not on strips.
'''
import numpy

# flow_locate_points: lambda_k >= POINT_TOL for all k (csrc/form_kernels.hip)
POINT_TOL = -1.0e-12
# cell bounding boxes are padded by this times their width + height: a point
# that passes the test lies within (1e-12 + rounding) * diameter of the cell
BOX_PAD = 1.0e-9


def as_points(points):
    '''(n, 2) float64 array of an (n, 2) array-like or a list of Points.'''
    if isinstance(points, (list, tuple)) and points and all(
            hasattr(p, 'xy') for p in points):
        points = [p.xy[:2] for p in points]
    pts = numpy.array(points, dtype=numpy.float64)
    if pts.size == 0:
        return numpy.zeros((0, 2))
    if pts.ndim != 2 or pts.shape[1] != 2:
        raise ValueError('points: an (n, 2) array or a list of Points, got '
                         'shape %r' % (pts.shape,))
    return numpy.ascontiguousarray(pts)


def barycentric(mesh, cells, pts):
    '''lambda (3, n) of pts (n, 2) on cells (n,), in the operation order of
    the kernel's test (csrc/form_kernels.hip: point_in_cell), which does not
    contract: the same bits.'''
    v = mesh.points[mesh.cell_vertices[cells]]          # (n, 3, 2)
    x0, x1, x2 = v[:, 0, 0], v[:, 1, 0], v[:, 2, 0]
    y0, y1, y2 = v[:, 0, 1], v[:, 1, 1], v[:, 2, 1]
    j00, j01, j10, j11 = x1 - x0, x2 - x0, y1 - y0, y2 - y0
    det = j00 * j11 - j01 * j10
    dx, dy = pts[:, 0] - x0, pts[:, 1] - y0
    l1 = (j11 * dx - j01 * dy) / det
    l2 = (j00 * dy - j10 * dx) / det
    l0 = 1.0 - l1 - l2
    return numpy.stack([l0, l1, l2])


class PointGrid(object):
    '''The bucket grid of a mesh (include/flow_hip.h, flow_point_grid), host
    arrays: nx * ny buckets over the bounding box, aspect following it,
    about `cells_per_bucket` cells per bucket; start (nb + 1,) and cells
    (start[nb],) int32, CSR, each bucket ascending.'''

    def __init__(self, mesh, cells_per_bucket=1.0):
        p = mesh.points
        nc = mesh.num_cells()
        lo, hi = p.min(axis=0), p.max(axis=0)
        ext = numpy.maximum(hi - lo, 1e-300)
        nb = max(1.0, nc / float(cells_per_bucket))
        nx = int(max(1, min(nb, round(numpy.sqrt(nb * ext[0] / ext[1])))))
        ny = int(max(1, round(nb / nx)))
        self.nx, self.ny = nx, ny
        self.x0, self.y0 = float(lo[0]), float(lo[1])
        self.hx_inv = float(nx / ext[0])
        self.hy_inv = float(ny / ext[1])
        # the padded bounding boxes and their bucket ranges
        v = p[mesh.cell_vertices]                       # (nc, 3, 2)
        blo, bhi = v.min(axis=1), v.max(axis=1)
        pad = BOX_PAD * (bhi - blo).sum(axis=1)
        blo = blo - pad[:, None]
        bhi = bhi + pad[:, None]
        i0, j0 = self.bucket_xy(blo)
        i1, j1 = self.bucket_xy(bhi)
        w = (i1 - i0 + 1).astype(numpy.int64)
        count = w * (j1 - j0 + 1)
        # one entry per (cell, bucket): repeat, then a stable sort by bucket
        # (the cells enter in ascending order and keep it within a bucket)
        cell = numpy.repeat(numpy.arange(nc, dtype=numpy.int64), count)
        first = numpy.cumsum(count) - count
        k = numpy.arange(len(cell), dtype=numpy.int64) - first[cell]
        ix = i0[cell] + k % w[cell]
        iy = j0[cell] + k // w[cell]
        bucket = iy * nx + ix
        order = numpy.argsort(bucket, kind='stable')
        self.cells = cell[order].astype(numpy.int32)
        start = numpy.zeros(nx * ny + 1, dtype=numpy.int64)
        numpy.cumsum(numpy.bincount(bucket, minlength=nx * ny), out=start[1:])
        assert start[-1] < 2**31
        self.start = start.astype(numpy.int32)

    def bucket_xy(self, pts):
        '''Bucket column and row of points (n, 2), clamped to the grid: the
        kernel's arithmetic (monotone in the coordinates, so a point inside
        a padded box falls in one of the box's buckets).'''
        tx = numpy.floor((pts[:, 0] - self.x0) * self.hx_inv)
        ty = numpy.floor((pts[:, 1] - self.y0) * self.hy_inv)
        tx = numpy.clip(numpy.nan_to_num(tx, nan=0.0), 0, self.nx - 1)
        ty = numpy.clip(numpy.nan_to_num(ty, nan=0.0), 0, self.ny - 1)
        return tx.astype(numpy.int64), ty.astype(numpy.int64)

    def bucket(self, pts):
        ix, iy = self.bucket_xy(pts)
        return iy * self.nx + ix

    def candidates(self, b):
        return self.cells[self.start[b]:self.start[b + 1]]

    def stats(self):
        '''(mean, max) candidates per bucket.'''
        per = numpy.diff(self.start)
        return float(per.mean()), int(per.max())


def point_grid(mesh):
    '''The mesh's bucket grid, built once (the geometry never changes).'''
    held = mesh._cache.get('point_grid')
    if held is None:
        held = mesh._cache['point_grid'] = PointGrid(mesh)
    return held


def _grid_struct(mesh):
    '''flow_point_grid of the mesh, uploaded once per device.'''
    from .. import _hip, device
    cache = mesh._cache.setdefault('point_grid_dev', {})
    key = str(device.get())
    held = cache.get(key)
    if held is None:
        g = point_grid(mesh)
        start, cells = device.to_device(g.start), device.to_device(g.cells)
        s = _hip.PointGridS(
            g.nx, g.ny, g.x0, g.y0, g.hx_inv, g.hy_inv,
            _hip.i32(start, len(g.start), 'grid start'),
            _hip.i32(cells, len(g.cells), 'grid cells'))
        held = cache[key] = (s, start, cells)
    return held[0]


class Probes(object):
    '''Values of fields at fixed points of a mesh.

        probes = Probes(mesh, [(0.15, 0.2), (0.25, 0.2)])
        probes(p)                   # numpy (n,) -- (n, 2) for a vector
        probes(sqrt(dot(u, u)))     # any rank <= 1 expression
        probes.evaluate(u, out=t)   # device (value_size, n), no host sync

    The points are located once, on the GPU, at construction: `.cells`
    (int32, -1 outside the mesh) and `.found` (bool).  Values at points
    outside are NaN.'''

    def __init__(self, mesh, points):
        import ctypes
        import torch
        from .. import _hip, device
        from .ops import _no_strips, mesh_struct
        _no_strips('Point evaluation')
        self.mesh = mesh
        self.points = as_points(points)
        n = len(self.points)
        self.n = n
        dev = device.get()
        self._xy = device.to_device(self.points.T.copy()) if n else None
        self._cell = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        self._bary = device.empty(max(3 * n, 1))
        if n:
            _hip.check(_hip.lib().flow_locate_points(
                ctypes.byref(mesh_struct(mesh)), ctypes.byref(_grid_struct(mesh)),
                n, _hip.f64(self._xy, 2 * n, 'points'),
                _hip.i32(self._cell, n, 'cells'),
                _hip.f64(self._bary, 3 * n, 'barycentric coordinates'),
                _hip.stream()))
        self.cells = device.to_host(self._cell).numpy()[:n].copy()
        self.found = self.cells >= 0

    def __len__(self):
        return self.n

    def evaluate(self, f, out=None):
        '''f at the points as a device fp64 tensor (value_size, n), written
        into `out` if given; enqueued on the package's stream, no host
        synchronisation.'''
        import ctypes
        from .. import _hip, device
        from . import forms
        from .ops import _form_struct, _no_strips, mesh_struct
        _no_strips('Point evaluation')
        expr = forms.as_form(f)
        forms._join_mesh(expr.mesh, self.mesh)
        prog = forms.point_program(expr)
        nout = prog.nout
        if out is None:
            out = device.empty(max(nout * self.n, 1))[:nout * self.n].view(
                nout, self.n)
        elif tuple(out.shape) != (nout, self.n):
            raise ValueError('out: shape %r, the values have shape %r'
                             % (tuple(out.shape), (nout, self.n)))
        if self.n:
            fs, keep = _form_struct(prog, self.mesh, 0)
            _hip.check(_hip.lib().flow_form_points(
                ctypes.byref(mesh_struct(self.mesh)), ctypes.byref(fs), self.n,
                _hip.i32(self._cell, self.n, 'cells'),
                _hip.f64(self._bary, 3 * self.n, 'barycentric coordinates'),
                _hip.f64(out, nout * self.n, 'out'), _hip.stream()))
            del keep
        return out

    def __call__(self, f):
        '''f at the points, on the host: (n,) for a scalar, (n, 2) for a
        vector; NaN at points outside the mesh.'''
        from .. import device
        vals = device.to_host(self.evaluate(f)).numpy()
        return vals[0].copy() if vals.shape[0] == 1 else vals.T.copy()


def evaluate_function(u, args):
    '''Function.__call__: u(x, y), u(Point(x, y)), u((x, y)),
    u(numpy.array([x, y])).  A float for a scalar field, a numpy (2,) array
    for a vector field; RuntimeError outside the mesh.'''
    if len(args) == 2:
        x = (args[0], args[1])
    elif len(args) == 1:
        x = args[0].xy[:2] if hasattr(args[0], 'xy') else args[0]
    else:
        raise TypeError('u(x, y), u(Point(x, y)) or u((x, y)): got %d '
                        'arguments' % len(args))
    x = numpy.asarray(x, dtype=numpy.float64).reshape(-1)
    if x.shape != (2,):
        raise ValueError('a point of the 2-D mesh has two coordinates, got %r'
                         % (x.tolist(),))
    probes = Probes(u.function_space().mesh(), x[None, :])
    if not probes.found[0]:
        raise RuntimeError('Unable to evaluate function at point (%r, %r): it '
                           'lies outside the mesh' % (x[0], x[1]))
    v = probes(u)[0]
    return float(v) if numpy.ndim(v) == 0 else v
