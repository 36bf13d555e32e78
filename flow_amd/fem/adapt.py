# -*- coding: utf-8 -*-
'''
Adaptive mesh refinement: estimate -> mark -> refine, the three steps that
produce the "other mesh" fem.Transfer carries a field to.

    J = JumpIndicator(V)
    eta2 = J.apply(u)                   # device, (nc,): one launch, no sync
    cells = mark(eta2, 0.5)             # host bool mask, one read-back
    fine = refine(mesh, cells)          # host, a new Mesh with parent_cell
    Transfer(V, FunctionSpace(fine, ...)).apply(u)

Indicator (flow_jump_indicator, csrc/adapt_kernels.hip): for a scalar or
2-vector P1 / P2 field the Kelly-type

    eta2[T] = sum over the interior edges E of T of
              |E| / 24 * int_E sum_k [grad u_k . n]^2 ds,

one lane per cell, every interior edge evaluated from both of its cells.  The
kernel finds a cell's neighbours through `facet_table(mesh)`, built here once
per mesh and uploaded once per device.

Marking: Doerfler's bulk criterion, a share of the maximum, or a share of
the cells; sort, cumulative sum and compare run where eta2 lives (torch on
the device, numpy for a host array), by the same rules.

Refinement: longest-edge bisection with conforming closure (Rivara's 4T-LE,
partial divisions included), vectorised numpy on the host.  The new mesh is
numbered by Mesh.reordered()'s rule and is an original (no vertex_origin /
cell_origin); a midpoint on the circle of a body-fitted hole is moved onto
the circle.

Not on strips.
'''
import math

import numpy

STRATEGIES = ('dorfler', 'maximum', 'fraction')

# a boundary edge belongs to the fitted hole when both end points lie within
# this many radii of its circle
ON_CIRCLE = 1.0e-9


# -- the neighbour table of the indicator kernel ------------------------------
def facet_table(mesh):
    '''(3 * nc,) int32, entry [i*nc + c] for local facet i of cell c: -1 on
    the boundary, else (n << 3) | (j << 1) | flip with n the cell across the
    facet, j the facet's local index in n and flip = 0 when the first vertex
    of n's facet j is the first vertex of c's facet i (the vertices of local
    facet k are k == 0 ? 1 : 0 and k == 2 ? 1 : 2), 1 when it is the second.
    Built once per mesh.'''
    held = mesh._cache.get('facet_table')
    if held is not None:
        return held
    nc = mesh.num_cells()
    if nc >= 1 << 28:
        raise ValueError('the facet table packs cell indices below 2**28; '
                         'the mesh has %d cells' % nc)
    nb = mesh.cell_neighbors.astype(numpy.int64)            # (nc, 3)
    ce = mesh.cell_edges
    cv = mesh.cell_vertices
    inner = nb >= 0
    n = numpy.where(inner, nb, 0)
    # the neighbour's local facet: where it lists the shared edge
    same = ce[n] == ce[:, :, None]                          # (nc, 3, 3)
    j = same.argmax(axis=2)
    assert (same.sum(axis=2)[inner] == 1).all()
    first = numpy.array([1, 0, 0])                          # facet_v0
    mine = cv[:, first]                                     # (nc, 3)
    theirs = cv[n, first[j]]
    flip = (mine != theirs).astype(numpy.int64)
    table = numpy.where(inner, (nb << 3) | (j << 1) | flip, -1)
    held = numpy.ascontiguousarray(table.T.reshape(-1).astype(numpy.int32))
    mesh._cache['facet_table'] = held
    return held


def _facet_table_dev(mesh):
    from .. import device
    cache = mesh._cache.setdefault('facet_table_dev', {})
    key = str(device.get())
    held = cache.get(key)
    if held is None:
        held = cache[key] = device.to_device(facet_table(mesh))
    return held


# -- the indicator ------------------------------------------------------------
class JumpIndicator(object):
    '''The jump indicator of Functions of V (scalar or 2-vector P1 / P2).

        J = JumpIndicator(V)
        eta2 = J.apply(u)           # device fp64 (nc,); enqueued, no sync
        J.apply(u, out=eta2)        # into eta2, returned
        J.estimate(u)               # sqrt(sum eta2), a float (synchronises)
    '''

    def __init__(self, V):
        from .ops import _no_strips
        if not hasattr(V, 'layout'):
            raise NotImplementedError(
                'V: a mixed space; take the indicator of its sub-spaces one '
                'by one')
        if getattr(V, 'component', None) is not None:
            raise NotImplementedError(
                'V: a component view (W.sub(i)); take the indicator of the '
                'vector field, or of a Function on W.sub(i).collapse()')
        if V.degree not in (1, 2):
            raise ValueError('V: P%r; the jump indicator takes P1 or P2'
                             % (V.degree,))
        if V.dim not in (1, 2):
            raise ValueError('V: %r components; scalar or 2-vector' % (V.dim,))
        _no_strips('The jump indicator')
        self.V = V
        self.nc = V.mesh().num_cells()
        facet_table(V.mesh())

    def apply(self, u, out=None):
        '''eta2 of the Function u on V: a new device tensor (nc,), or `out`
        (a contiguous device fp64 tensor of nc entries), which is returned.
        One kernel launch on the package's stream.'''
        import ctypes
        from .. import _hip, device
        from .function import Function
        from .ops import _no_strips, mesh_struct, space_struct
        _no_strips('The jump indicator')
        if not isinstance(u, Function) \
                or not u.function_space().same_as(self.V):
            raise ValueError('u: not a Function of the space this indicator '
                             'was built for')
        lib = _hip.lib()
        nc, V = self.nc, self.V
        if out is None:
            out = device.empty(nc)
        elif getattr(out, 'shape', None) != (nc,):
            raise ValueError('out: a device fp64 tensor of shape (%d,)' % nc)
        table = _facet_table_dev(V.mesh())
        _hip.check(lib.flow_jump_indicator(
            ctypes.byref(mesh_struct(V.mesh())),
            ctypes.byref(space_struct(V.layout)), V.dim,
            _hip.i32(table, 3 * nc, 'facet table'),
            _hip.f64(u.data, V.dim * V.N, 'u'), _hip.f64(out, nc, 'eta2'),
            _hip.stream()))
        return out

    def estimate(self, u):
        '''sqrt(sum eta2): the estimate of the whole mesh, a float.'''
        from .. import device
        total = self.apply(u).sum()
        return math.sqrt(float(device.to_host(total)))


def jump_indicator(u):
    '''JumpIndicator(u.function_space()).apply(u), for a single use.'''
    return JumpIndicator(u.function_space()).apply(u)


# -- marking ------------------------------------------------------------------
def mark(eta2, fraction, strategy='dorfler'):
    '''The cells to refine, a host bool array (nc,), from their eta2 (a torch
    tensor, on the device or not, or a numpy array).

      'dorfler'   the smallest set whose eta2 sum is at least fraction * the
                  total: cells in descending order (stable: ties by index)
                  while the sum of those before is below the target;
      'maximum'   eta2 >= fraction * max(eta2);
      'fraction'  the first ceil(fraction * nc) cells of that order.

    A tensor is sorted, summed and compared where it lives, and the mask is
    read back once.'''
    if strategy not in STRATEGIES:
        raise ValueError('strategy %r: one of %s' % (strategy, STRATEGIES))
    fraction = float(fraction)
    if not 0.0 < fraction <= 1.0:
        raise ValueError('fraction %r: in (0, 1]' % (fraction,))
    if isinstance(eta2, numpy.ndarray):
        return _mark_numpy(eta2, fraction, strategy)
    import torch
    if not isinstance(eta2, torch.Tensor):
        raise ValueError('eta2: a torch tensor or a numpy array')
    return _mark_torch(eta2, fraction, strategy)


def _count(fraction, nc):
    return min(nc, int(math.ceil(fraction * nc)))


def _mark_numpy(eta2, fraction, strategy):
    eta2 = numpy.asarray(eta2, dtype=numpy.float64)
    if eta2.ndim != 1 or len(eta2) == 0:
        raise ValueError('eta2: one value per cell')
    if numpy.isnan(eta2).any():
        raise ValueError('eta2 holds NaNs')
    nc = len(eta2)
    if strategy == 'maximum':
        return eta2 >= fraction * eta2.max()
    order = numpy.argsort(-eta2, kind='stable')
    if strategy == 'fraction':
        chosen = numpy.arange(nc) < _count(fraction, nc)
    else:
        total = numpy.cumsum(eta2[order])
        before = numpy.concatenate([[0.0], total[:-1]])
        chosen = before < fraction * total[-1]
    mask = numpy.zeros(nc, dtype=bool)
    mask[order] = chosen
    return mask


def _mark_torch(eta2, fraction, strategy):
    import torch
    from .. import device
    if eta2.dim() != 1 or eta2.numel() == 0:
        raise ValueError('eta2: one value per cell')
    eta2 = eta2.to(torch.float64)
    nc = eta2.numel()
    if strategy == 'maximum':
        mask = eta2 >= fraction * eta2.max()
    else:
        sorted_, order = torch.sort(eta2, descending=True, stable=True)
        if strategy == 'fraction':
            chosen = torch.arange(nc, device=eta2.device) < _count(fraction, nc)
        else:
            total = torch.cumsum(sorted_, 0)
            before = torch.cat([total.new_zeros(1), total[:-1]])
            chosen = before < fraction * total[-1]
        mask = torch.zeros(nc, dtype=torch.bool, device=eta2.device)
        mask[order] = chosen
    # the NaN flag travels with the mask: one read-back
    both = torch.cat([mask, torch.isnan(eta2).any().reshape(1)])
    host = device.to_host(both).numpy()
    if host[-1]:
        raise ValueError('eta2 holds NaNs')
    return host[:-1].copy()


# -- refinement ---------------------------------------------------------------
def _signed_areas(points, cells):
    p = points[cells]
    d1, d2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    return 0.5 * (d1[:, 0] * d2[:, 1] - d1[:, 1] * d2[:, 0])


def marked_edges(mesh, markers):
    '''(edge mask (ne,), local index of every cell's longest edge (nc,)):
    all three edges of every marked cell, closed: while a cell has a marked
    edge but its longest edge is not marked, that one is marked too.  The
    longest edge: exact comparison of the squared lengths (one value per
    EDGE, so both of its cells see the same), ties to the lowest edge id.'''
    p = mesh.points
    ce = mesh.cell_edges.astype(numpy.int64)
    d = p[mesh.edges[:, 0]] - p[mesh.edges[:, 1]]
    len2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]
    l2 = len2[ce]
    longest = numpy.zeros(len(ce), dtype=numpy.int64)
    best_l2, best_e = l2[:, 0].copy(), ce[:, 0].copy()
    for k in (1, 2):
        better = (l2[:, k] > best_l2) | ((l2[:, k] == best_l2) & (ce[:, k] < best_e))
        longest[better] = k
        best_l2[better] = l2[better, k]
        best_e[better] = ce[better, k]
    em = numpy.zeros(len(mesh.edges), dtype=bool)
    em[ce[markers].ravel()] = True
    while True:                     # sweeps of the closure, not cells
        need = em[ce].any(axis=1) & ~em[best_e]
        if not need.any():
            break
        em[best_e[need]] = True
    return em, longest


def refine(mesh, markers=None):
    '''The mesh with the marked cells (a bool array (nc,); None: all) refined
    by longest-edge bisection with conforming closure.  Every marked edge
    gets one midpoint; a cell is split by its pattern, the longest edge L
    first: L alone 2 children, L and one other edge j 3 (m_j joined to m_L),
    all three 4 (m_L joined to both other midpoints); a marked cell has all
    three.  Children keep the parent's orientation.  Returns a new Mesh,
    numbered by Mesh.reordered()'s rule, with `parent_cell` (nc_new,) int64
    in that numbering; vertex_origin / cell_origin are None, `hole` is
    carried over and new midpoints of the hole's edges are moved onto its
    circle (not where a child cell would lose its area or turn over).'''
    from .mesh import Mesh
    nc, nv = mesh.num_cells(), mesh.num_vertices()
    if markers is None:
        markers = numpy.ones(nc, dtype=bool)
    else:
        markers = numpy.asarray(markers)
        if markers.dtype != numpy.bool_:
            raise ValueError('markers: a bool array, one entry per cell (got '
                             'dtype %s)' % markers.dtype)
        if markers.shape != (nc,):
            raise ValueError('markers: shape %r, the mesh has %d cells'
                             % (markers.shape, nc))
    em, longest = marked_edges(mesh, markers)
    edges = mesh.edges.astype(numpy.int64)
    mid = numpy.full(len(edges), -1, dtype=numpy.int64)
    split = numpy.nonzero(em)[0]
    mid[split] = nv + numpy.arange(len(split))
    p = mesh.points
    chord = 0.5 * (p[edges[split, 0]] + p[edges[split, 1]])
    points = numpy.concatenate([p, chord])
    # every cell turned so that its longest edge is local edge 0 (a cyclic
    # shift keeps the orientation): r0 faces L = (r1, r2)
    rot = (longest[:, None] + numpy.arange(3)[None, :]) % 3
    rows = numpy.arange(nc)[:, None]
    r = mesh.cell_vertices.astype(numpy.int64)[rows, rot]
    m = mid[mesh.cell_edges.astype(numpy.int64)[rows, rot]]
    r0, r1, r2 = r[:, 0], r[:, 1], r[:, 2]
    mL, m1, m2 = m[:, 0], m[:, 1], m[:, 2]      # on (r1,r2), (r2,r0), (r0,r1)
    hasL, has1, has2 = mL >= 0, m1 >= 0, m2 >= 0
    assert (hasL | ~(has1 | has2)).all(), 'closure'

    def tri(a, b, c):
        return numpy.stack([a, b, c], axis=1)

    # the bisection of L gives (r0, r1, mL) and (r0, mL, r2); each half is
    # bisected once more when its other edge of the parent is marked
    slots = numpy.stack([
        tri(r0, r1, r2),
        tri(r0, r1, mL), tri(r0, m2, mL), tri(m2, r1, mL),
        tri(r0, mL, r2), tri(r0, mL, m1), tri(m1, mL, r2),
        ], axis=1)                                              # (nc, 7, 3)
    valid = numpy.stack([
        ~hasL,
        hasL & ~has2, hasL & has2, hasL & has2,
        hasL & ~has1, hasL & has1, hasL & has1,
        ], axis=1)
    cells = slots[valid]
    parent = numpy.repeat(numpy.arange(nc, dtype=numpy.int64), 7)[valid.ravel()]
    if mesh.hole is not None and len(split):
        orient = numpy.sign(_signed_areas(p, mesh.cell_vertices))[parent]
        points = _snap_to_hole(mesh, points, cells, orient, split, nv)
    out = Mesh(points, cells.astype(numpy.int32))
    out.hole = mesh.hole
    out = out.reordered()
    out.parent_cell = parent[out.cell_origin]
    out.vertex_origin = out.cell_origin = None
    return out


def refined_markers(markers, fine_mesh):
    '''The cell MeshFunction `markers` of a mesh carried to the mesh
    refine() made of it: every child cell gets its parent's value
    (fine_mesh.parent_cell), so a material map survives estimate -> mark ->
    refine.  Host only; needs forms.cell_subdomains(True) like every cell
    MeshFunction.'''
    from .mesh import MeshFunction
    if getattr(markers, 'dim', None) != 2:
        raise ValueError('refined_markers takes a cell MeshFunction (dim 2)')
    parent = getattr(fine_mesh, 'parent_cell', None)
    if parent is None:
        raise ValueError('refined_markers: the fine mesh has no parent_cell '
                         '(it is not the result of refine())')
    if len(parent) != fine_mesh.num_cells() or (
            len(parent) and parent.max() >= markers.size()):
        raise ValueError('refined_markers: the fine mesh was not refined '
                         'from the mesh of the markers')
    out = MeshFunction(markers.value_type, fine_mesh, 2)
    out.set_where(numpy.ones(fine_mesh.num_cells(), dtype=bool),
                  markers.array()[parent])
    return out


def _snap_to_hole(mesh, points, cells, orient, split, nv):
    '''The midpoints of split boundary edges with both end points on the
    hole's circle, moved radially onto it; a midpoint some child cell of
    which would lose its area or turn over (orient: the sign of its parent's
    signed area) stays on the chord.'''
    cx, cy, radius = mesh.hole
    centre = numpy.array([cx, cy])
    is_b = numpy.zeros(len(mesh.edges), dtype=bool)
    is_b[mesh.bfacets] = True
    ends = mesh.points[mesh.edges[split]] - centre          # (ns, 2, 2)
    off = numpy.abs(numpy.hypot(ends[:, :, 0], ends[:, :, 1]) - radius)
    on = is_b[split] & (off <= ON_CIRCLE * radius).all(axis=1)
    ids = nv + numpy.nonzero(on)[0]
    chord = points[ids].copy()
    d = chord - centre
    snapped = points.copy()
    snapped[ids] = centre + d * (radius / numpy.hypot(d[:, 0], d[:, 1]))[:, None]
    moved = numpy.zeros(len(points), dtype=bool)
    moved[ids] = True
    while moved.any():              # sweeps: the moved set only shrinks
        bad = _signed_areas(snapped, cells) * orient <= 0.0
        back = numpy.zeros(len(points), dtype=bool)
        back[cells[bad].ravel()] = True
        back &= moved
        if not back.any():
            break
        snapped[back] = points[back]
        moved &= ~back
    return snapped
