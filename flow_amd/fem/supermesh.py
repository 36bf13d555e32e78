# -*- coding: utf-8 -*-
'''
Error norms and inner products between discrete fields that live on
different meshes,

    S = Supermesh(V_a, V_b)
    eta2 = S.cell_errors(u, w)          # device (nc_b,): per cell of V_b's mesh
    S.errornorm(u, w, 'H1')             # a float
    S.inner(u, w)                       # a float
    S.coverage, S.min_coverage, S.area, S.pairs

with u a Function of V_a and w a Function of V_b, scalar or 2-vector P1 / P2
with the same number of components; the two meshes may differ or be one
mesh.  This is what a mesh-convergence study of a flow without an analytic
solution needs (a coarse run against a fine one), and the denominator of an
estimator's effectivity index.  errornorm() takes an Expression on one
mesh; Transfer followed by a norm on one mesh adds an interpolation error
of the order of the one to be measured; assemble() refuses the fields of
two meshes.

The integrals run over the SUPERMESH, the intersections of every cell of
V_b's mesh (the target, as in Projection: the result lives on its cells)
with the cells of V_a's mesh under it.  On every intersection polygon
(u - w)^2 has degree <= 4 and |grad u - grad w|^2 degree <= 2, so the
7-point degree-5 rule on the fanned polygon is exact: the norms carry no
interpolation and no quadrature error, only rounding.

Pair list: projection.pair_list, on the host, once.  Kernel
(flow_supermesh_norms, csrc/projection_kernels.hip, next to the clipping it
shares with Projection): one target cell per lane walks its row of the list
in order and leaves two values per cell, the value plane and the gradient
plane; in product mode u w and grad u . grad w take the place of the squared
differences.  The sums over the cells are done on the device in a fixed
order.  No atomics: two calls give the same bits.

Coverage: as for Projection, from the same geometry launch.  Without
allow_partial a target cell covered below 1 - 1e-10 is a ValueError.  With it
the integrals run over the overlap of the two meshes as it is -- nothing is
rescaled, an uncovered cell contributes 0 -- and `area` is the covered area.

Rounding.  A cell of V_a's mesh that shares only an edge with the target
cell may leave a sliver of area ~eps |cell|.  u - w is continuous across it
and contributes nothing; grad u - grad w jumps there, so where the two
fields agree the 'H10' values stop at ~eps |cell| |jump of the gradient|^2,
not at 0 (relative to |u|_1^2: ~1e-16).

Construction uploads the pair list, runs the geometry once and reads the
coverage back: the only synchronisation.  cell_errors() is one launch and
waits for nothing; errornorm() and inner() wait for their two sums.  Not on
strips.
'''
import math

import numpy

from .projection import FULL, pair_list
from .transfer import _scalar_or_vector

NORMS = ('L2', 'H10', 'H1')


def _norm_type(norm_type):
    if norm_type not in NORMS:
        raise ValueError('norm_type %r: one of %s' % (norm_type, NORMS))
    return norm_type


class Supermesh(object):
    '''Norms of u - w and products of u and w, for Functions u of V_a and w
    of V_b, set up once.

        S = Supermesh(V_a, V_b, allow_partial=False)
        S.cell_errors(u, w, norm_type='L2', out=None)   # device (nc_b,)
        S.errornorm(u, w, norm_type='L2')               # a float
        S.inner(u, w, norm_type='L2')                   # a float
        S.coverage                  # device (nc_b,): covered share per cell
        S.min_coverage, S.area, S.pairs

    norm_type: 'L2' the values, 'H10' the gradients, 'H1' both.'''

    def __init__(self, V_a, V_b, allow_partial=False):
        import ctypes
        from .. import _hip, device
        from .ops import _no_strips, mesh_struct
        _scalar_or_vector(V_a, 'V_a')
        _scalar_or_vector(V_b, 'V_b')
        if V_a.dim != V_b.dim:
            raise ValueError('V_a has %d component(s), V_b %d'
                             % (V_a.dim, V_b.dim))
        _no_strips('Norms across meshes')
        self.V_a, self.V_b = V_a, V_b
        self.allow_partial = bool(allow_partial)
        mesh_a, mesh_b = V_a.mesh(), V_b.mesh()
        nc = self.nc = mesh_b.num_cells()
        pptr, psrc = pair_list(mesh_a, mesh_b)
        self.pairs = len(psrc)
        lib = _hip.lib()
        self._pptr = device.to_device(pptr)
        # (an empty list still needs an address)
        self._psrc = device.to_device(psrc if len(psrc) else
                                      numpy.zeros(1, dtype=numpy.int32))
        self.coverage = device.empty(nc)
        # the geometry launch of Projection
        _hip.check(lib.flow_project_load(
            ctypes.byref(mesh_struct(mesh_a)), None,
            ctypes.byref(mesh_struct(mesh_b)), None, V_b.dim,
            _hip.i32(self._pptr, nc + 1, 'pptr'),
            _hip.i32(self._psrc, self.pairs, 'psrc'), self.pairs, None, 0, None,
            _hip.f64(self.coverage, nc, 'coverage'), None, _hip.stream()))
        cov = device.to_host(self.coverage).numpy()[:nc]
        self.min_coverage = float(cov.min())
        self.area = float((cov * mesh_b.cell_areas()).sum())
        part = ~(cov >= FULL)
        if part.any() and not self.allow_partial:
            raise ValueError(
                '%d of %d target cells are not covered by the source mesh '
                '(the worst coverage: %r); allow_partial=True integrates over '
                'the overlap of the two meshes' % (int(part.sum()), nc,
                                                   self.min_coverage))

    def _check(self, u, w):
        from .function import Function
        if not isinstance(u, Function) \
                or not u.function_space().same_as(self.V_a):
            raise ValueError('u: not a Function of the first space of this '
                             'Supermesh (V_a)')
        if not isinstance(w, Function) \
                or not w.function_space().same_as(self.V_b):
            raise ValueError('w: not a Function of the second space of this '
                             'Supermesh (V_b)')

    def _cell_values(self, u, w, product=False, totals=False, psrc=None,
                     values=None, work=None):
        '''(values, totals): the device buffer (2 * nc_b,) of the value plane
        and the gradient plane, and their two sums (host floats; None
        without `totals`, and then nothing is waited for).  psrc: another
        pair list of the same length; values, work: the buffers to use (the
        tests' guard checks).'''
        import ctypes
        from .. import _hip, device
        from .ops import _no_strips, mesh_struct, space_struct
        from .ops import work as work_buffer
        _no_strips('Norms across meshes')
        self._check(u, w)
        V_a, V_b, nc = self.V_a, self.V_b, self.nc
        if values is None:
            values = device.empty(2 * nc)
        host = (ctypes.c_double * 2)() if totals else None
        if totals and work is None:
            work = work_buffer(_hip.REDUCE_WORK)
        _hip.check(_hip.lib().flow_supermesh_norms(
            ctypes.byref(mesh_struct(V_a.mesh())),
            ctypes.byref(space_struct(V_a.layout)),
            ctypes.byref(mesh_struct(V_b.mesh())),
            ctypes.byref(space_struct(V_b.layout)), V_b.dim,
            _hip.i32(self._pptr, nc + 1, 'pptr'),
            _hip.i32(self._psrc if psrc is None else psrc, self.pairs, 'psrc'),
            self.pairs, _hip.f64(u.data, V_a.size(), 'u'),
            _hip.f64(w.data, V_b.size(), 'w'), int(bool(product)),
            _hip.f64(values, 2 * nc, 'cell values'),
            _hip.f64(work, _hip.REDUCE_WORK, 'work') if totals else None,
            host, _hip.stream()))
        return values, ((host[0], host[1]) if totals else None)

    def cell_errors(self, u, w, norm_type='L2', out=None):
        '''The squared error per cell of V_b's mesh, a device fp64 tensor
        (nc_b,): 'L2' sum_comp int (u - w)^2 over the part of the cell that
        V_a's mesh covers, 'H10' the same of |grad u - grad w|^2, 'H1' their
        sum.  A new tensor, or `out` (a contiguous device fp64 tensor of nc_b
        entries), which is returned.  One kernel launch on the package's
        stream (both planes; picking or adding them is torch's), no
        synchronisation.  What fem.mark takes.'''
        import torch
        _norm_type(norm_type)
        nc = self.nc
        if out is not None and getattr(out, 'shape', None) != (nc,):
            raise ValueError('out: a device fp64 tensor of shape (%d,)' % nc)
        values, _ = self._cell_values(u, w)
        if norm_type == 'H1':
            return torch.add(values[:nc], values[nc:], out=out)
        plane = values[:nc] if norm_type == 'L2' else values[nc:]
        return plane if out is None else out.copy_(plane)

    @staticmethod
    def _pick(totals, norm_type):
        if norm_type == 'L2':
            return totals[0]
        if norm_type == 'H10':
            return totals[1]
        return totals[0] + totals[1]

    def errornorm(self, u, w, norm_type='L2'):
        '''sqrt of the sum over the cells of cell_errors(u, w, norm_type), a
        float.  The cells of each plane are summed on the device in a fixed
        order (include/flow_hip.h: flow_supermesh_norms); 'H1' is sqrt(the
        'L2' sum + the 'H10' sum).  Waits for the stream.'''
        _norm_type(norm_type)
        _, totals = self._cell_values(u, w, totals=True)
        return math.sqrt(self._pick(totals, norm_type))

    def inner(self, u, w, norm_type='L2'):
        '''sum_comp int u w ('L2'), int grad u . grad w ('H10') or both
        ('H1') over the overlap of the two meshes, a float: correlations
        between runs, and with u twice (V_a and V_b one space) its squared
        norm on the overlap.  The same kernel in product mode, the same
        sums.'''
        _norm_type(norm_type)
        _, totals = self._cell_values(u, w, product=True, totals=True)
        return self._pick(totals, norm_type)


def mesh_errornorm(u, w, norm_type='L2', allow_partial=False):
    '''Supermesh(u.function_space(), w.function_space()).errornorm(u, w),
    for a single use: the norm of u - w for Functions of two meshes.'''
    from .function import Function
    _norm_type(norm_type)
    for name, f in (('u', u), ('w', w)):
        if not isinstance(f, Function):
            raise ValueError('%s: not a Function (errornorm() takes '
                             'expressions)' % name)
    return Supermesh(u.function_space(), w.function_space(),
                     allow_partial=allow_partial).errornorm(u, w, norm_type)
