# -*- coding: utf-8 -*-
'''
Contour lines and level-set measures of a nodal field on the GPU: where is
f == c, how long is that line, and how large is {f >= c}?

    I = Isolines(V)                  # V: scalar P1 or P2 space
    C = I.extract(f, levels)         # f: Function on V; levels: a float or a
                                     # sequence of floats
    C.nseg                           # number of segments (the one host
                                     # read-back of an extract)
    C.xy                             # device fp64 (nseg, 4): x0, y0, x1, y1
    C.level                          # device int32 (nseg,): index into levels
    C.cell                           # device int32 (nseg,): parent cell
    C.keys                           # device int32 (nseg, 4): the dofs (a0, b0,
                                     # a1, b1) of the two crossed sub-edges,
                                     # a < b
    C.bary                           # device fp64 (nseg, 2, 3): barycentric
                                     # coordinates of both end points in the
                                     # parent cell
    C.polylines(k=None)              # host: ordered vertex arrays per level,
                                     # each with a closed flag
    C.evaluate(expr, t=0.5)          # device (ncomp, nseg): an expression
                                     # (anything Probes.evaluate takes) on
                                     # every segment at parameter t in [0, 1]
    I.length(f, levels)              # numpy (nlevels,): length of {f_h == c}
    I.area(f, levels)                # numpy (nlevels,): area of {f_h >= c}
    isolines(f, levels)              # Isolines(f.function_space()).extract(...)

What is contoured.  f_h, the continuous piecewise-LINEAR interpolant of the
nodal values of f: linear on every triangle of the P1 triangulation of the
dofs (csrc/subtri.h).  On P1 that is the field itself.  On P2 the contour is
that of f_h, NOT of the quadratic, so its position is second order in the mesh
width -- what a plot of the nodal values shows, at the resolution of the dofs.

Definitions (csrc/isoline_kernels.hip; tests/isolines_reference.py restates
them in numpy).

  * A node is ABOVE iff f >= c.  A sub-triangle emits a segment iff its nodes
    are not all on one side.  One case is taken out: the one node above lies
    exactly on the level -- both crossings are then that node, the segment
    would have no length, and nothing is emitted (nothing is lost from a
    length or an area; where such a node ends a ridge of nodes on the level,
    the chain of keys is cut there although the coordinates still meet).  So
    a field equal to c everywhere emits nothing, and a node on the level
    yields neither a zero-length nor a duplicate segment.
  * A crossing is computed from the lower dof of its sub-edge (a, b), a < b,
    towards the higher (subtri.h's rule), so the two cells at an edge produce
    the same bits, and `keys` carries (a, b): polylines are chained on
    integers.
  * A segment has the above side on its left: chained lines have one
    orientation, a closed contour round a maximum is counter-clockwise.
  * A sub-triangle with a non-finite nodal value (Distance yields inf) emits
    nothing and adds nothing to a length or an area.
  * Segments are ordered by cell, then level index, then sub-triangle (the
    corners at v0, v1, v2, then the middle): two calls give the same bits in
    every output.  Lengths and areas are block sums added in a fixed order on
    a grid that depends on the number of cells alone: the same bits, too.

Levels travel with the launches, ISOLINE_LEVELS_PER_LAUNCH at a time; nothing
is uploaded per call.  extract() counts (one launch per 32 levels), scans the
counts with torch (cumsum in int64: plumbing), reads the total back once and
emits (one launch per 32 levels); with no segment nothing is allocated and
nothing more is launched.  Not on strips.
'''
import numpy

from . import ops
from ._levelset import field_on, scalar_p12_space

INT32_MAX = 2**31 - 1


def _levels(levels):
    '''levels as a float64 array (nlevels,); ValueError where there is none
    or one is not finite.'''
    try:
        arr = numpy.atleast_1d(numpy.asarray(levels, dtype=numpy.float64))
    except (TypeError, ValueError):
        raise ValueError('levels: a float or a sequence of floats, got %r'
                         % (levels,))
    if arr.ndim != 1 or arr.size == 0:
        raise ValueError('levels: a float or a non-empty sequence of floats, '
                         'got shape %r' % (arr.shape,))
    if not numpy.isfinite(arr).all():
        raise ValueError('levels: every level must be finite, got %r'
                         % (arr.tolist(),))
    return numpy.ascontiguousarray(arr)


def _launches(levels):
    '''The flow_isoline_levels structs of the launches that cover `levels`.'''
    from .. import _hip
    per = _hip.ISOLINE_LEVELS_PER_LAUNCH
    out = []
    for base in range(0, len(levels), per):
        s = _hip.IsolineLevels()
        part = levels[base:base + per]
        s.n, s.base = len(part), base
        for k, c in enumerate(part):
            s.c[k] = float(c)
        out.append(s)
    return out


def chain_segments(keys, level, nlevels):
    '''Join segments into polylines on their integer keys.

    keys (nseg, 4): (a0, b0) names the sub-edge a segment starts on, (a1, b1)
    the one it ends on; level (nseg,): its level index.  Per level every key
    starts at most one segment and ends at most one (a repeated key keeps
    its first segment).  Returns, per level, a list of (indices, closed):
    `indices` the segments of one line in the direction of the segments
    (the above side stays on the left).  Open lines come first, each from
    the segment whose start key ends no segment -- the end that lies on a
    boundary sub-edge -- in ascending order of that key; then the closed
    lines, each from its smallest start key, in ascending order of it.'''
    keys = numpy.asarray(keys, dtype=numpy.int64).reshape(-1, 4)
    level = numpy.asarray(level, dtype=numpy.int64).reshape(-1)
    if len(keys) != len(level):
        raise ValueError('chain_segments: %d keys, %d levels'
                         % (len(keys), len(level)))
    lines = [[] for _ in range(int(nlevels))]
    for k in range(int(nlevels)):
        idx = numpy.nonzero(level == k)[0]
        if len(idx) == 0:
            continue
        start = [tuple(r) for r in keys[idx, 0:2].tolist()]
        end = [tuple(r) for r in keys[idx, 2:4].tolist()]
        by_start, ends = {}, set()
        for i, s in enumerate(start):
            by_start.setdefault(s, i)
        ends.update(end)
        order = sorted(range(len(idx)), key=lambda i: start[i])
        seen = numpy.zeros(len(idx), dtype=bool)

        def follow(i):
            line = []
            while i is not None and not seen[i]:
                seen[i] = True
                line.append(i)
                i = by_start.get(end[i])
            return line, i

        for i in order:                       # open lines
            if not seen[i] and start[i] not in ends:
                line, _ = follow(i)
                lines[k].append((idx[line], False))
        for i in order:                       # closed ones
            if not seen[i]:
                line, back = follow(i)
                lines[k].append((idx[line], back == line[0]))
    return lines


class Contours(object):
    '''The segments of one Isolines.extract(); see the module's text.'''

    def __init__(self, V, levels, nseg, xy, level, cell, keys, bary):
        self.V = V
        self.levels = levels
        self.nseg = int(nseg)
        self.xy, self.level, self.cell = xy, level, cell
        self.keys, self.bary = keys, bary

    def polylines(self, k=None):
        '''The contour as polylines, on the host (one read-back of xy, keys
        and level): per level a list of (vertices (m, 2), closed).  An open
        line of s segments has s + 1 vertices; a closed one s, the first not
        repeated.  k: that level's list alone.'''
        from .. import device
        nl = len(self.levels)
        if k is not None and not 0 <= int(k) < nl:
            raise ValueError('k: %r, there are %d levels' % (k, nl))
        if self.nseg == 0:
            out = [[] for _ in range(nl)]
        else:
            xy = device.to_host(self.xy).numpy()
            keys = device.to_host(self.keys).numpy()
            level = device.to_host(self.level).numpy()
            out = []
            for lines in chain_segments(keys, level, nl):
                per = []
                for idx, closed in lines:
                    pts = xy[idx, 0:2] if closed else numpy.concatenate(
                        [xy[idx, 0:2], xy[idx[-1:], 2:4]])
                    per.append((pts.copy(), bool(closed)))
                out.append(per)
        return out if k is None else out[int(k)]

    def evaluate(self, expr, t=0.5):
        '''expr on every segment at x0 + t (x1 - x0): a device fp64 tensor
        (value_size, nseg); no host synchronisation.  The two barycentric
        triples are interpolated and flow_form_points runs the expression's
        program in the parent cells.'''
        import ctypes
        from .. import _hip, device
        from . import forms
        t = float(t)
        if not 0.0 <= t <= 1.0:
            raise ValueError('t: %r is outside [0, 1]' % (t,))
        ops._no_strips('Isolines')
        mesh = self.V.mesh()
        form = forms.as_form(expr)
        forms._join_mesh(form.mesh, mesh)
        prog = forms.point_program(form)
        nout, n = prog.nout, self.nseg
        out = device.empty(max(nout * n, 1))[:nout * n].view(nout, n)
        if n:
            lam = (self.bary[:, 0, :] * (1.0 - t) + self.bary[:, 1, :] * t) \
                .t().contiguous()
            fs, keep = ops._form_struct(prog, mesh, 0)
            _hip.check(_hip.lib().flow_form_points(
                ctypes.byref(ops.mesh_struct(mesh)), ctypes.byref(fs), n,
                _hip.i32(self.cell, n, 'cells'),
                _hip.f64(lam, 3 * n, 'barycentric coordinates'),
                _hip.f64(out, nout * n, 'out'), _hip.stream()))
            del keep
        return out


class Isolines(object):
    '''Contour lines, their length and the area above them for Functions on
    the scalar P1 / P2 space V; see the module's text.'''

    def __init__(self, V):
        scalar_p12_space(V, 'contour a Function on',
                         'contours are those of a scalar field', 'Isolines')
        ops._no_strips('Isolines')
        self.V = V
        self._work = None

    def _structs(self):
        import ctypes
        V = self.V
        return (ctypes.byref(ops.mesh_struct(V.mesh())),
                ctypes.byref(ops.space_struct(V.layout)))

    def extract(self, f, levels):
        '''The segments of {f_h == c} for every c in levels, as Contours.'''
        import ctypes
        import torch
        from .. import _hip, device
        f = field_on(self.V, f, 'f', 'these isolines were')
        levels = _levels(levels)
        ops._no_strips('Isolines')
        lib = _hip.lib()
        V = self.V
        nc = V.mesh().num_cells()
        mesh_s, space_s = self._structs()
        fp = _hip.f64(f.data, V.N, 'f')
        launches = _launches(levels)
        dev = device.get()
        counts = torch.empty((len(launches), nc), dtype=torch.int32, device=dev)
        for j, L in enumerate(launches):
            _hip.check(lib.flow_isoline_count(
                mesh_s, space_s, fp, ctypes.byref(L),
                _hip.i32(counts[j], nc, 'count'), _hip.stream()))
        # the scan: per cell its launches one behind the other, cells in order
        wide = counts.to(torch.int64)
        per_cell = wide.sum(dim=0)
        ends = torch.cumsum(per_cell, dim=0)
        total = int(device.to_host(ends[-1:])[0])
        if total == 0:
            e = torch.empty
            return Contours(
                V, levels, 0, e((0, 4), dtype=torch.float64, device=dev),
                e((0,), dtype=torch.int32, device=dev),
                e((0,), dtype=torch.int32, device=dev),
                e((0, 4), dtype=torch.int32, device=dev),
                e((0, 2, 3), dtype=torch.float64, device=dev))
        if total > INT32_MAX:
            raise ValueError(
                'isolines: %d segments, more than 2^31 - 1: take fewer levels '
                'per call' % total)
        offsets = ((ends - per_cell).unsqueeze(0)
                   + torch.cumsum(wide, dim=0) - wide).to(torch.int32)
        xy = device.empty(4 * total).view(total, 4)
        bary = device.empty(6 * total).view(total, 2, 3)
        level = torch.empty(total, dtype=torch.int32, device=dev)
        cell = torch.empty(total, dtype=torch.int32, device=dev)
        keys = torch.empty((total, 4), dtype=torch.int32, device=dev)
        for j, L in enumerate(launches):
            _hip.check(lib.flow_isoline_emit(
                mesh_s, space_s, fp, ctypes.byref(L),
                _hip.i32(counts[j], nc, 'count'),
                _hip.i32(offsets[j], nc, 'offset'), total,
                _hip.f64(xy, 4 * total, 'xy'), _hip.i32(level, total, 'level'),
                _hip.i32(cell, total, 'cell'),
                _hip.i32(keys, 4 * total, 'keys'),
                _hip.f64(bary, 6 * total, 'bary'), _hip.stream()))
        return Contours(V, levels, total, xy, level, cell, keys, bary)

    def _measure(self, f, levels):
        '''numpy (nlevels, 2): length and area per level; one read-back.'''
        import ctypes
        from .. import _hip, device
        f = field_on(self.V, f, 'f', 'these isolines were')
        levels = _levels(levels)
        ops._no_strips('Isolines')
        lib = _hip.lib()
        V = self.V
        nc = V.mesh().num_cells()
        per = _hip.ISOLINE_LEVELS_PER_LAUNCH
        nblocks = (nc + 255) // 256
        if self._work is None:
            self._work = device.empty(2 * per * nblocks)
        mesh_s, space_s = self._structs()
        out = device.empty(2 * len(levels))
        for L in _launches(levels):
            _hip.check(lib.flow_isoline_measure(
                mesh_s, space_s, _hip.f64(f.data, V.N, 'f'), ctypes.byref(L),
                _hip.f64(self._work, 2 * L.n * nblocks, 'partials'),
                _hip.f64(out[2 * L.base:], 2 * L.n, 'out'), _hip.stream()))
        return device.to_host(out).numpy().reshape(len(levels), 2).copy()

    def length(self, f, levels):
        '''numpy (nlevels,): the length of {f_h == c} for every level.'''
        return self._measure(f, levels)[:, 0].copy()

    def area(self, f, levels):
        '''numpy (nlevels,): the area of {f_h >= c} for every level.'''
        return self._measure(f, levels)[:, 1].copy()


def isolines(f, levels):
    '''Isolines(f.function_space()).extract(f, levels), for a single use.'''
    from .function import Function
    if not isinstance(f, Function):
        raise ValueError('f: a Function on a scalar P1 or P2 space, got %r'
                         % (type(f),))
    return Isolines(f.function_space()).extract(f, levels)
