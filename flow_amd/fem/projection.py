# -*- coding: utf-8 -*-
'''
Conservative transfer between meshes: the L2 (Galerkin) projection of a
discrete field of one mesh into a space of another,

    P = Projection(V_from, V_to)
    P.apply(u_from, out=w)          # w in V_to: (w, v) = (u_from, v) for all v
    b = P.load(u_from)              # the right-hand side alone
    P.coverage, P.min_coverage, P.pairs

between scalar or 2-vector P1 / P2 spaces of the same number of components.
Where Transfer interpolates (the value of u_from at every node of V_to),
this is the field of V_to nearest to u_from in L2: it keeps int u dx (1 lies
in V_to), which interpolation does not, and does not alias when the target
is the coarser mesh.  It is the transfer step of estimate -> mark -> refine
-> transfer -> solve.  Like every Galerkin projection it over- and
undershoots at fronts the target mesh cannot resolve; nothing here limits
it.

The right-hand side b_i = int phi_i^to u_from dx needs the intersections of
every target cell with the source cells under it (the supermesh).

Pair list (host, once; pair_list below): per target cell, ascending, the
source cells whose padded bounding box overlaps the target cell's padded
bounding box, found through the source mesh's PointGrid.  A superset of the
pairs that meet; the order fixes the order of every sum.

Kernel (flow_project_load, csrc/projection_kernels.hip): one target cell per
lane clips each listed source triangle to its own (Sutherland-Hodgman), fans
the polygon and integrates with the 7-point degree-5 rule, which is exact
for the integrand (degree <= 4); the gather over the target space's vector
contribution map sums the cells' results.  No atomics: the same bits on
every call.

Mass solve: the mass matrix of V_to (cached on the space), per component,
with the solver of project(): CG + Jacobi to `rtol`.

Coverage.  Two meshes of one domain approximate a curved boundary by
different polygons, so a target cell may be covered by source cells only in
part, or not at all.  `coverage` (device, one entry per target cell) is the
covered share of each cell's area, from the same clips.  Without
allow_partial a cell below 1 - 1e-10 is a ValueError.  With it the cell's
contribution is divided by its coverage -- the mean of u_from over the
covered part stands for the rest -- and int u dx is then kept only UP TO THE
UNCOVERED AREA: int w dx = the sum over the target cells T of |T| times the
mean of u_from over the covered part of T (not pointwise: a constant comes
back as a constant only in the mean of each cell), and what of the source
mesh lies outside the target mesh is lost.  A cell with coverage 0 has no
such mean and is a ValueError in any case.

Construction uploads the pair list, runs the geometry once and reads
min_coverage back: the only synchronisation.  apply() and load() upload
nothing; load() waits for nothing, apply() for the convergence checks of
its mass solves.  Not on strips.
'''
import numpy

from .points import BOX_PAD, point_grid
from .transfer import _scalar_or_vector

# a target cell counts as covered from here on (rounding of the clips and the
# area sums is ~1e-15)
FULL = 1.0 - 1.0e-10


def padded_boxes(mesh):
    '''(lo, hi), each (nc, 2): the cells' bounding boxes, padded as PointGrid
    pads them.'''
    v = mesh.points[mesh.cell_vertices]                 # (nc, 3, 2)
    lo, hi = v.min(axis=1), v.max(axis=1)
    pad = BOX_PAD * (hi - lo).sum(axis=1)
    return lo - pad[:, None], hi + pad[:, None]


# target cells per pass of pair_list: bounds its temporaries (some tens of
# entries of 8 bytes per target cell and array)
PAIR_CHUNK = 1 << 18


def pair_list(mesh_from, mesh_to):
    '''(pptr (nc_to + 1,), psrc) int32, CSR: per cell of mesh_to, ascending
    and without repeats, the cells of mesh_from whose padded bounding box
    overlaps its padded bounding box.  Vectorised: the buckets of the source
    mesh's PointGrid under the target box, their cells, the union, the box
    test.  (A source cell is listed in every bucket its padded box touches
    and bucket_xy is monotone, so two overlapping boxes share a bucket.)'''
    g = point_grid(mesh_from)
    nc_from, nc_to = mesh_from.num_cells(), mesh_to.num_cells()
    slo, shi = padded_boxes(mesh_from)
    tlo, thi = padded_boxes(mesh_to)
    start = g.start.astype(numpy.int64)
    per_cell = numpy.zeros(nc_to, dtype=numpy.int64)
    found = []
    for c0 in range(0, nc_to, PAIR_CHUNK):
        c1 = min(c0 + PAIR_CHUNK, nc_to)
        i0, j0 = g.bucket_xy(tlo[c0:c1])
        i1, j1 = g.bucket_xy(thi[c0:c1])
        w = (i1 - i0 + 1).astype(numpy.int64)
        count = w * (j1 - j0 + 1)
        # one entry per (target cell, bucket) ...
        tgt = numpy.repeat(numpy.arange(c1 - c0, dtype=numpy.int64), count)
        k = numpy.arange(len(tgt), dtype=numpy.int64) \
            - (numpy.cumsum(count) - count)[tgt]
        bucket = (j0[tgt] + k // w[tgt]) * g.nx + i0[tgt] + k % w[tgt]
        # ... then per (target cell, cell of that bucket)
        per = start[bucket + 1] - start[bucket]
        tgt2 = numpy.repeat(tgt, per)
        k2 = numpy.arange(len(tgt2), dtype=numpy.int64) - numpy.repeat(
            numpy.cumsum(per) - per, per)
        src = g.cells[numpy.repeat(start[bucket], per) + k2].astype(numpy.int64)
        key = numpy.unique(tgt2 * nc_from + src)        # ascending (target, source)
        t, s = c0 + key // nc_from, key % nc_from
        keep = ((tlo[t] <= shi[s]) & (slo[s] <= thi[t])).all(axis=1)
        per_cell[c0:c1] = numpy.bincount(t[keep] - c0, minlength=c1 - c0)
        found.append(s[keep].astype(numpy.int32))
    pptr = numpy.zeros(nc_to + 1, dtype=numpy.int64)
    numpy.cumsum(per_cell, out=pptr[1:])
    if pptr[-1] >= 2**31:
        raise ValueError('%d candidate cell pairs: the pair list holds fewer '
                         'than 2**31' % pptr[-1])
    psrc = numpy.concatenate(found) if found else numpy.zeros(0, numpy.int32)
    return pptr.astype(numpy.int32), psrc


class Projection(object):
    '''The L2 projection of Functions of V_from into V_to, set up once.

        P = Projection(V_from, V_to, allow_partial=False, rtol=1e-12)
        w = P.apply(u)              # a Function on V_to
        P.apply(u, out=w)           # into w, which is returned
        b = P.load(u)               # device (V_to.size(),): int phi_i u dx
        P.coverage                  # device (nc_to,): covered share per cell
        P.min_coverage, P.pairs     # a float, an int

    int w dx = int u dx for every component where the source mesh covers
    every target cell and lies within the target mesh.  With allow_partial
    partly covered cells are scaled by 1 / coverage and conservation holds
    up to the uncovered area (the module's text); `coverage` tells where.
    A Galerkin projection is not bounded by the range of u: it overshoots
    at fronts.'''

    def __init__(self, V_from, V_to, allow_partial=False, rtol=1.0e-12):
        import ctypes
        from .. import _hip, device
        from .ops import _no_strips, mesh_struct
        _scalar_or_vector(V_from, 'V_from')
        _scalar_or_vector(V_to, 'V_to')
        if V_from.dim != V_to.dim:
            raise ValueError('V_from has %d component(s), V_to %d'
                             % (V_from.dim, V_to.dim))
        _no_strips('Field projection')
        self.V_from, self.V_to = V_from, V_to
        self.allow_partial = bool(allow_partial)
        self.rtol = float(rtol)
        mesh_from, mesh_to = V_from.mesh(), V_to.mesh()
        nc = self.nc = mesh_to.num_cells()
        pptr, psrc = pair_list(mesh_from, mesh_to)
        self.pairs = len(psrc)
        lib = _hip.lib()
        self._pptr = device.to_device(pptr)
        # (an empty list still needs an address)
        self._psrc = device.to_device(psrc if len(psrc) else
                                      numpy.zeros(1, dtype=numpy.int32))
        self.coverage = device.empty(nc)
        _hip.check(lib.flow_project_load(
            ctypes.byref(mesh_struct(mesh_from)), None,
            ctypes.byref(mesh_struct(mesh_to)), None, V_to.dim,
            _hip.i32(self._pptr, nc + 1, 'pptr'),
            _hip.i32(self._psrc, self.pairs, 'psrc'), self.pairs, None, 0, None,
            _hip.f64(self.coverage, nc, 'coverage'), None, _hip.stream()))
        cov = device.to_host(self.coverage).numpy()[:nc]
        self.min_coverage = float(cov.min())
        part = ~(cov >= FULL)
        if part.any() and not self.allow_partial:
            raise ValueError(
                '%d of %d target cells are not covered by the source mesh '
                '(the worst coverage: %r); allow_partial=True scales them by '
                '1 / coverage' % (int(part.sum()), nc, self.min_coverage))
        none = ~(cov > 0.0)
        if none.any():
            raise ValueError(
                '%d of %d target cells have coverage 0 (or none defined): no '
                'part of the source mesh lies in them' % (int(none.sum()), nc))

    def _check_u(self, u_from):
        from .function import Function
        if not isinstance(u_from, Function) \
                or not u_from.function_space().same_as(self.V_from):
            raise ValueError('u_from: not a Function of the space this '
                             'Projection reads (V_from)')

    def _load(self, u_from, b, psrc=None):
        '''b = the load vector of u_from; psrc: another pair list of the
        same length (the tests' guarded-read check).'''
        import ctypes
        from .. import _hip
        from .ops import mesh_struct, scratch, space_struct
        V_from, V_to = self.V_from, self.V_to
        lay, nc, dim = V_to.layout, self.nc, V_to.dim
        buf = scratch(V_to.mesh(), dim * lay.nloc * nc)
        _hip.check(_hip.lib().flow_project_load(
            ctypes.byref(mesh_struct(V_from.mesh())),
            ctypes.byref(space_struct(V_from.layout)),
            ctypes.byref(mesh_struct(V_to.mesh())),
            ctypes.byref(space_struct(lay)), dim,
            _hip.i32(self._pptr, nc + 1, 'pptr'),
            _hip.i32(self._psrc if psrc is None else psrc, self.pairs, 'psrc'),
            self.pairs, _hip.f64(u_from.data, V_from.size(), 'u_from'),
            int(self.allow_partial),
            _hip.f64(buf, dim * lay.nloc * nc, 'scratch'),
            _hip.f64(self.coverage, nc, 'coverage'),
            _hip.f64(b, V_to.size(), 'b'), _hip.stream()))
        return b

    def load(self, u_from):
        '''b[a * N + i] = int phi_i u_from_a dx over the target mesh (scaled
        per cell with allow_partial): a new device vector of V_to.size()
        entries.  Two launches on the package's stream, no synchronisation.'''
        from .. import device
        from .ops import _no_strips
        _no_strips('Field projection')
        self._check_u(u_from)
        return self._load(u_from, device.empty(self.V_to.size()))

    def apply(self, u_from, out=None):
        '''The projection of u_from (a Function on V_from) into V_to: a new
        Function, or `out` (a Function on V_to), which is returned.  The load
        vector, then one mass solve per component from a zero start.'''
        from .. import _hip, device
        from .function import Function
        from .ops import _no_strips, assemble_mass, krylov_solve
        _no_strips('Field projection')
        self._check_u(u_from)
        V = self.V_to
        if out is None:
            out = Function(V)
        elif not isinstance(out, Function) \
                or not out.function_space().same_as(V):
            raise ValueError('out: not a Function of the space this '
                             'Projection writes (V_to)')
        elif out.data.data_ptr() == u_from.data.data_ptr():
            raise ValueError('out: the source field itself')
        else:
            _hip.fill(out.data, 0.0)
        b = self._load(u_from, device.empty(V.size()))
        M = assemble_mass(V)
        key = ('M_dinv',)
        if key not in V.layout._dev:
            V.layout._dev[key] = M.diag_inv()
        n = V.N
        for a in range(V.dim):
            krylov_solve('cg', M, b[a * n:(a + 1) * n], out.data[a * n:(a + 1) * n],
                         self.rtol, maxit=1000, dinv=V.layout._dev[key],
                         check_every=10)
        return out


def project_onto(u, V, allow_partial=False, rtol=1.0e-12):
    '''Projection(u.function_space(), V).apply(u), for a single use.'''
    from .function import Function
    if not isinstance(u, Function):
        raise ValueError('u: not a Function (project() takes expressions)')
    return Projection(u.function_space(), V, allow_partial=allow_partial,
                      rtol=rtol).apply(u)
