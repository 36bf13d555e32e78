# -*- coding: utf-8 -*-
'''
Connected components of a level set on the GPU, with measures per component:
how many vortices are there, where is each one and how strong is it?

    R = Regions(V)                       # V: scalar P1 or P2 space
    C = R.label(f, level, side='above')  # f: Function on V; level: finite float
                                         # 'above': inside iff f >= level
                                         #          (Isolines' rule)
                                         # 'below': inside iff f <  level
    C.count        # int: number of components
    C.sweeps       # sweeps run, a multiple of CHECK_EVERY
    C.labels       # device int32 (V.N,): component id 0..count-1, -1 outside
    C.root         # device int32 (count,): smallest dof of each component;
                   # ids ascend with it
    C.size         # device int32 (count,): number of dofs
    C.area         # device fp64 (count,): area of the component's part of
                   # {f_h inside}
    C.centroid     # device fp64 (count, 2)
    C.integrate(g) # device fp64 (ncomp, count): the integral of g over each
                   # component; g a P1 / P2 Function (scalar or 2-vector) on
                   # the same mesh, of any degree
    C.extrema(g)   # (min, max), each device fp64 (ncomp, count), over the
                   # component's dofs; g on V or on the vector space of V's
                   # degree
    C.as_function()# Function on V holding float(labels): a form operand,
                   # conditional(eq(ind, k), w, 0)*dx
    C.mask(k)      # Function on V: 1.0 on component k, else 0.0
    regions(f, level, side='above')      # Regions(f.function_space()).label(..)

Definitions (csrc/region_kernels.hip; tests/regions_reference.py restates them
in numpy).

  * The graph is the P1 triangulation of the dofs (csrc/subtri.h), Isolines'
    and Distance's.  The two vertices of a P2 edge are therefore no
    neighbours: the mid point lies between them.
  * A dof with a non-finite value is outside.  Two inside dofs joined by a
    sub-edge are in one component; since f_h is linear on a sub-triangle these
    are exactly the components of {f_h >= c}.  A component's label is its
    smallest dof, compact ids ascend with it, and nothing depends on an
    ordering of the work.
  * A sub-triangle with no inside dof, or with a non-finite value, adds no
    piece.  With 3 inside dofs the piece is the sub-triangle, with 1 the
    corner at that node, with 2 (A, B inside, C outside) the quadrilateral A,
    B, Q, P, P on A-C and Q on B-C, cut by the diagonal A-Q.  Crossings are
    Isolines', by the one rule of subtri.h.  All inside dofs of a
    sub-triangle share a component, which owns the piece; the four
    sub-triangles of a P2 cell may belong to different components.
  * Per piece the integrals of 1, x, y and g_a, g the true P1 / P2 polynomial
    of the parent cell, by the edge-midpoint rule on each triangle of the
    piece (exact for degree 2); areas as absolute values; centroid =
    (int x, int y) / area, NaN for a component without a piece (all its
    sub-triangles hold a non-finite value) or with pieces of no area.

label() initialises (one launch), enqueues CHECK_EVERY sweeps at a time and
reads one integer back per batch, as Distance.apply does; a sweep takes the
minimum label over a dof and its inside neighbours and follows it once
(new[i] = old[m]: the reach doubles per sweep along a monotonically numbered
path).  Compact ids are torch plumbing on ints (a cumsum of labels == arange,
a gather); the count is the one further scalar read back.  The pieces of one
launch are then sorted by owner (torch.sort, stable; searchsorted gives the
segments) and summed per component by one block per (component, row) in a
fixed order: two calls give the same bits.  With no component nothing after
the initialisation and one batch of sweeps is launched.

Limits.  What is measured is the piecewise-LINEAR f_h, not the quadratic; the
components are those of the sub-edge graph; components are not tracked from
one time step to the next; not on strips.
'''
import numpy

from . import ops
from ._levelset import field_on, scalar_p12_space, sweep_to_fixed_point

# sweeps per batch, one read-back of the flag behind each: of 4, 8 and 32 on
# the bench mesh the fastest on P2 and level with 4 on P1 (DESIGN.md, section
# 3, "Regions", has the table)
CHECK_EVERY = 8

SIDES = {'above': 0, 'below': 1}


def segment_offsets(sorted_keys, count):
    '''offsets (count + 1,) int32 of the segments of equal keys in a sorted
    int tensor: key k fills [offsets[k], offsets[k + 1]); keys below 0 come
    first and belong to no segment.'''
    import torch
    want = torch.arange(int(count) + 1, dtype=sorted_keys.dtype,
                        device=sorted_keys.device)
    return torch.searchsorted(sorted_keys.contiguous(), want).to(torch.int32)


def _sorted_segments(keys, count):
    '''(perm int32, offsets int32) of a stable sort of the keys.'''
    import torch
    skeys, perm = torch.sort(keys, stable=True)
    return perm.to(torch.int32), segment_offsets(skeys, count)


class Components(object):
    '''The components of one Regions.label(); see the module's text.'''

    def __init__(self, regions, f, level, side, count, sweeps, labels, root,
                 size, area, centroid, dof_perm, dof_offsets, slot_perm,
                 slot_offsets):
        self._regions = regions
        self.V = regions.V
        self._f, self.level, self.side = f, level, side
        self.count, self.sweeps = int(count), int(sweeps)
        self.labels, self.root, self.size = labels, root, size
        self.area, self.centroid = area, centroid
        self._dof_perm, self._dof_offsets = dof_perm, dof_offsets
        self._slot_perm, self._slot_offsets = slot_perm, slot_offsets

    def _operand(self, g, what):
        from .function import Function
        if not isinstance(g, Function):
            raise ValueError('g: a P1 or P2 Function on the mesh of these '
                             'regions, got %r' % (type(g),))
        W = g.function_space()
        if W.mesh() is not self.V.mesh():
            raise ValueError('g: a Function on another mesh')
        if getattr(W, 'component', None) is not None \
                or W.degree not in (1, 2) or W.dim not in (1, 2):
            raise ValueError('g: %s takes a scalar or 2-vector P1 / P2 '
                             'Function' % what)
        return W

    def integrate(self, g):
        '''The integral of g over every component: device fp64 (ncomp,
        count); no host synchronisation.  The pieces are cut again from f,
        which must still hold the values label() saw.'''
        import torch
        from .. import device
        W = self._operand(g, 'integrate')
        ops._no_strips('Regions')
        out = torch.empty((W.dim, self.count), dtype=torch.float64,
                          device=device.get())
        if self.count:
            R = self._regions
            vals = R._moments(self._f, self.level, self.labels, g, None)
            R._segment_sum(self.count, self._slot_offsets, self._slot_perm,
                           vals[3:], out)
        return out

    def extrema(self, g):
        '''(min, max) of the nodal values of g over the dofs of every
        component, each device fp64 (ncomp, count).'''
        import torch
        from .. import _hip, device
        W = self._operand(g, 'extrema')
        if W.degree != self.V.degree:
            raise ValueError('g: extrema runs over the dofs of V: a Function '
                             'on V or on the vector space of its degree')
        ops._no_strips('Regions')
        dev = device.get()
        lo = torch.empty((W.dim, self.count), dtype=torch.float64, device=dev)
        hi = torch.empty((W.dim, self.count), dtype=torch.float64, device=dev)
        if self.count:
            N = self.V.N
            _hip.check(_hip.lib().flow_region_segment_minmax(
                self.count, _hip.i32(self._dof_offsets, self.count + 1, 'offsets'),
                _hip.i32(self._dof_perm, N, 'perm'), W.dim, N,
                _hip.f64(g.data, W.dim * N, 'g'),
                _hip.f64(lo, W.dim * self.count, 'min'),
                _hip.f64(hi, W.dim * self.count, 'max'), _hip.stream()))
        return lo, hi

    def as_function(self):
        '''A Function on V holding float(labels).'''
        import torch
        from .function import Function
        return Function(self.V, self.labels.to(torch.float64))

    def mask(self, k):
        '''A Function on V: 1.0 on component k, else 0.0.'''
        import torch
        from .function import Function
        if not 0 <= int(k) < self.count:
            raise ValueError('k: %r, there are %d components' % (k, self.count))
        return Function(self.V, (self.labels == int(k)).to(torch.float64))


class Regions(object):
    '''The connected components of {f >= level} (or {f < level}) for
    Functions on the scalar P1 / P2 space V; see the module's text.  The two
    label buffers, the flag, the keys and the pieces' integrals are allocated
    once.'''

    def __init__(self, V):
        scalar_p12_space(V, 'label a Function on',
                         'regions are those of a scalar field', 'Regions')
        ops._no_strips('Regions')
        self.V = V
        self.nslots = (1 if V.degree == 1 else 4) * V.mesh().num_cells()
        self._dev = None

    def _buffers(self):
        '''(label buffer a, b, flag, keys, integrals of the pieces).'''
        import torch
        from .. import device
        if self._dev is None:
            dev = device.get()
            self._dev = (torch.empty(self.V.N, dtype=torch.int32, device=dev),
                         torch.empty(self.V.N, dtype=torch.int32, device=dev),
                         torch.zeros(1, dtype=torch.int32, device=dev),
                         torch.empty(self.nslots, dtype=torch.int32, device=dev),
                         device.empty(5 * self.nslots).view(5, self.nslots))
        return self._dev

    def _structs(self):
        return (ops.mesh_struct(self.V.mesh()),
                ops.space_struct(self.V.layout))

    def _moments(self, f, level, ids, g, keys):
        '''Launch flow_region_moments; the (3 + ncomp, nslots) integrals.'''
        import ctypes
        from .. import _hip
        mesh_s, space_s = self._structs()
        V = self.V
        vals = self._buffers()[4]
        if g is None:
            ncomp, G, gp = 0, None, None
        else:
            W = g.function_space()
            ncomp = W.dim
            G = ctypes.byref(ops.space_struct(W.layout))
            gp = _hip.f64(g.data, ncomp * W.N, 'g')
        _hip.check(_hip.lib().flow_region_moments(
            ctypes.byref(mesh_s), ctypes.byref(space_s),
            _hip.f64(f.data, V.N, 'f'), float(level),
            _hip.i32(ids, V.N, 'ids'), G, ncomp, gp,
            None if keys is None else _hip.i32(keys, self.nslots, 'keys'),
            _hip.f64(vals, (3 + ncomp) * self.nslots, 'integrals'),
            _hip.stream()))
        return vals[:3 + ncomp]

    def _segment_sum(self, count, offsets, perm, vals, out):
        from .. import _hip
        nrows = vals.shape[0]
        _hip.check(_hip.lib().flow_region_segment_sum(
            count, _hip.i32(offsets, count + 1, 'offsets'),
            _hip.i32(perm, self.nslots, 'perm'), nrows, self.nslots,
            _hip.f64(vals, nrows * self.nslots, 'integrals'),
            _hip.f64(out, nrows * count, 'out'), _hip.stream()))

    def label(self, f, level, side='above'):
        '''The components of {f >= level} ('above') or {f < level} ('below')
        as Components.  CHECK_EVERY sweeps per batch and one read-back of the
        flag behind each; _hip.NotConverged after more than V.N sweeps.'''
        import ctypes
        import torch
        from .. import _hip, device
        f = field_on(self.V, f, 'f', 'these regions were')
        try:
            level = float(level)
        except (TypeError, ValueError):
            raise ValueError('level: a finite float, got %r' % (level,))
        if not numpy.isfinite(level):
            raise ValueError('level: must be finite, got %r' % (level,))
        if side not in SIDES:
            raise ValueError("side: 'above' or 'below', got %r" % (side,))
        ops._no_strips('Regions')
        lib = _hip.lib()
        V, N = self.V, self.V.N
        a, b, flag, keys, _ = self._buffers()
        mesh_s, space_s = self._structs()
        _hip.check(lib.flow_region_init(
            ctypes.byref(space_s), _hip.f64(f.data, N, 'f'), level,
            SIDES[side], _hip.i32(a, N, 'labels'), _hip.stream()))

        def enqueue(a, b, nsweeps):
            _hip.check(lib.flow_region_sweeps(
                ctypes.byref(mesh_s), ctypes.byref(space_s), nsweeps,
                _hip.i32(a, N, 'label buffer'), _hip.i32(b, N, 'label buffer'),
                _hip.i32(flag, 1, 'flag'), _hip.stream()))

        a, b, sweeps = sweep_to_fixed_point(
            enqueue, a, b, flag, CHECK_EVERY, N, 'regions')
        # compact ids: plumbing on ints
        dev = device.get()
        is_root = a == torch.arange(N, dtype=torch.int32, device=dev)
        rank = torch.cumsum(is_root.to(torch.int64), dim=0)
        count = int(device.to_host(rank[-1:])[0])
        e = torch.empty
        if count == 0:
            return Components(
                self, f, level, side, 0, sweeps,
                torch.full((N,), -1, dtype=torch.int32, device=dev),
                e((0,), dtype=torch.int32, device=dev),
                e((0,), dtype=torch.int32, device=dev),
                e((0,), dtype=torch.float64, device=dev),
                e((0, 2), dtype=torch.float64, device=dev), None, None, None,
                None)
        inside = a >= 0
        ids = torch.where(
            inside, rank[a.clamp(min=0).to(torch.int64)] - 1,
            torch.full_like(rank, -1)).to(torch.int32)
        root = torch.nonzero(is_root)[:, 0].to(torch.int32)
        dof_perm, dof_offsets = _sorted_segments(ids, count)
        size = dof_offsets[1:] - dof_offsets[:-1]
        vals = self._moments(f, level, ids, None, keys)
        slot_perm, slot_offsets = _sorted_segments(keys, count)
        sums = device.empty(3 * count).view(3, count)
        self._segment_sum(count, slot_offsets, slot_perm, vals, sums)
        area = sums[0].clone()
        centroid = (sums[1:3] / sums[0:1]).t().contiguous()
        return Components(self, f, level, side, count, sweeps, ids, root,
                          size, area, centroid, dof_perm, dof_offsets,
                          slot_perm, slot_offsets)


def regions(f, level, side='above'):
    '''Regions(f.function_space()).label(f, level, side), for a single use.'''
    from .function import Function
    if not isinstance(f, Function):
        raise ValueError('f: a Function on a scalar P1 or P2 space, got %r'
                         % (type(f),))
    return Regions(f.function_space()).label(f, level, side)
