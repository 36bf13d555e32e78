# -*- coding: utf-8 -*-
'''
The distance to the wall (or to any set of dofs) as a nodal field, by a
monotone Eikonal solver on the mesh: |grad d| = 1, d = 0 at the sources.

    D = Distance(V, sources='on_boundary')   # V: scalar P1 or P2
    d = D.apply(out=None)       # a Function on V: >= 0, +inf where no path of
                                # cells leads to a source
    D.sweeps                    # Jacobi sweeps the last apply() ran
    wall_distance(V, sources='on_boundary')  # Distance(V, sources).apply()

sources:

    'on_boundary'       every exterior facet;
    a SubDomain         the exterior facets it marks, by DirichletBC's rule
                        (inside(x, True) at both vertices and the mid point);
    (markers, id)       the exterior facets with markers == id, markers a
                        MeshFunction('size_t', mesh, 1) / FacetFunction, as
                        ds(id) reads it;
    an integer array    dof indices of V;
    a bool array (V.N)  a mask over the dofs of V.

The dofs of a facet are its two vertices and, on P2, its mid point (of the
straight edge: cells are affine).  Source dofs get 0, every other dof starts
at +inf.

Scheme (flow_distance_sweeps, csrc/distance_kernels.hip).  The graph is the
P1 triangulation of the dofs (csrc/subtri.h).  A node C is updated from a
triangle (C, A, B) by the Hopf-Lax formula (Bornemann and Rasch): the minimum
over the edge A-B of T(x) + |C - x|, T linear on the edge -- the two end points
and, where there is one, the interior stationary point.  The end points keep
the update monotone and 1-Lipschitz on obtuse triangles too.  A sweep is
Jacobi between two buffers,

    new[i] = min(old[i], min over the triangles at i of the update of i),

one lane per dof over the node's row of the space's vector contribution map,
without atomics; the iteration ends when a sweep changes nothing, at the
greatest fixed point, which depends on no ordering: two calls give the same
bits.  apply() enqueues CHECK_EVERY sweeps at a time and reads one integer
back per batch (set by the batch's LAST sweep where it lowered a value), so
`sweeps` is the number the fixed point needs -- the sweep that confirms it
included -- rounded up to a multiple of CHECK_EVERY.

Limits.  First order: the error is O(h) and grows with the distance.  The
distance is to the source POLYGON (the dofs on it and the straight edges
between them), not to the circle it approximates.  The number of sweeps grows
with the diameter of the mesh counted in cells: information moves one layer of
nodes per sweep.  Not on strips.
'''
import numpy

from . import ops
from ._levelset import field_on, scalar_p12_space, sweep_to_fixed_point

# sweeps per batch, one read-back of the flag behind each: the fastest of 8, 32
# and 128 on the bench mesh, P1 and P2 ("Wall distance",
# has the table and what it does not show)
CHECK_EVERY = 128


def _facet_dofs(V, facets):
    '''Dofs of V on the facets (edge ids): vertices and (P2) mid points.'''
    mesh, layout = V.mesh(), V.layout
    dofs = [layout.vertex_dofs[mesh.edges[facets].ravel()]]
    if layout.degree == 2:
        dofs.append(layout.edge_dofs[facets])
    return numpy.concatenate(dofs)


def source_dofs(V, sources):
    '''The sorted unique dof indices (int64) a `sources` argument selects in
    the scalar space V; ValueError where it selects none.'''
    from .bcs import facet_marked
    from .mesh import MeshFunction
    mesh = V.mesh()
    bf = mesh.bfacets
    if isinstance(sources, str) or hasattr(sources, 'inside'):
        if isinstance(sources, str) and sources != 'on_boundary':
            raise ValueError("sources: %r; the only string is 'on_boundary'"
                             % (sources,))
        dofs = _facet_dofs(V, bf[facet_marked(sources, mesh, bf, True)])
    elif isinstance(sources, tuple) and len(sources) == 2 \
            and isinstance(sources[0], MeshFunction):
        markers, value = sources
        if markers.mesh is not mesh:
            raise ValueError('sources: the facet markers belong to another '
                             'mesh')
        dofs = _facet_dofs(V, bf[markers.array()[bf] == value])
    else:
        arr = numpy.asarray(sources)
        if arr.dtype == numpy.bool_:
            if arr.shape != (V.N,):
                raise ValueError('sources: a mask of shape %r, the space has '
                                 '%d dofs' % (arr.shape, V.N))
            dofs = numpy.nonzero(arr)[0]
        elif arr.ndim == 1 and arr.dtype.kind in 'iu':
            dofs = arr.astype(numpy.int64)
            if len(dofs) and (dofs.min() < 0 or dofs.max() >= V.N):
                raise ValueError('sources: dof indices outside [0, %d)' % V.N)
        else:
            raise ValueError(
                "sources: 'on_boundary', a SubDomain, a pair (facet markers, "
                'id), an integer array of dof indices or a bool mask over '
                'the dofs')
    dofs = numpy.unique(dofs).astype(numpy.int64)
    if len(dofs) == 0:
        raise ValueError('sources: no dof selected')
    return dofs


class Distance(object):
    '''The distance to `sources` on the scalar P1 / P2 space V; see the
    module's text.  The two buffers and the flag are allocated once.'''

    def __init__(self, V, sources='on_boundary'):
        scalar_p12_space(V, 'take the distance on',
                         'the distance is a scalar field', 'the wall distance',
                         ValueError)
        ops._no_strips('Wall distance')
        self.V = V
        self.dofs = source_dofs(V, sources)
        self.sweeps = 0
        V.layout.vmap('vptr')
        self._dev = None

    def _buffers(self):
        '''(start values, buffer a, buffer b, flag) on the device.'''
        import torch
        from .. import device
        if self._dev is None:
            start = numpy.full(self.V.N, numpy.inf)
            start[self.dofs] = 0.0
            self._dev = (device.to_device(start), device.empty(self.V.N),
                         device.empty(self.V.N),
                         device.zeros(1, dtype=torch.int32))
        return self._dev

    def apply(self, out=None):
        '''The distance as a new Function on V, or written into `out` (a
        Function on V), which is returned.  CHECK_EVERY sweeps per batch on
        the package's stream and one read-back of the flag behind each;
        _hip.NotConverged after more than V.N + CHECK_EVERY sweeps (no dof
        changes more often than V.N times).'''
        import ctypes
        from .. import _hip
        from .function import Function
        ops._no_strips('Wall distance')
        V, N = self.V, self.V.N
        if out is not None:
            field_on(V, out, 'out', 'this distance was')
        lib = _hip.lib()
        start, a, b, flag = self._buffers()
        mesh_s = ops.mesh_struct(V.mesh())
        space_s = ops.space_struct(V.layout)

        def enqueue(a, b, nsweeps):
            _hip.check(lib.flow_distance_sweeps(
                ctypes.byref(mesh_s), ctypes.byref(space_s), nsweeps,
                _hip.f64(a, N, 'distance buffer'),
                _hip.f64(b, N, 'distance buffer'),
                _hip.i32(flag, 1, 'flag'), _hip.stream()))

        _hip.copy(a, start)
        self.sweeps = 0
        a, b, self.sweeps = sweep_to_fixed_point(
            enqueue, a, b, flag, CHECK_EVERY, N, 'wall distance')
        if out is None:
            out = Function(V)
        _hip.copy(out.data, a)
        return out


def wall_distance(V, sources='on_boundary'):
    '''Distance(V, sources).apply(), for a single use.'''
    return Distance(V, sources).apply()
