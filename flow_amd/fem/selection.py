# -*- coding: utf-8 -*-
'''
What a measure with a subdomain selects -- ds(k), dS(k), dx(k) -- and what the
list launches of form assembly read of it: the marker checks, the host
selections, the device lists, the contribution maps, and the ONE cache rule all
of them are held by (held).  ops re-exports the public names; space.RectLayout
builds its maps with by_target.

Numpy, the device module and mesh data only: nothing here knows a form or the
library.
'''
import collections

import numpy

from .. import device


def is_cell_subdomain(part):
    '''Whether a part is a dx(k) part: cells, and a subdomain id.'''
    return part.integral_type == 'cell' \
        and part.subdomain_id not in (None, 'everywhere')


# -- marker checks: one per domain kind ----------------------------------------
def _check_facet_markers(mesh, markers, subdomain_id, measure='ds'):
    '''ds(k) | dS(k): markers where an id selects, of this mesh.'''
    if markers is None:
        if subdomain_id not in (None, 'everywhere'):
            raise ValueError(
                '%s(%r) needs markers: Measure(\'%s\', domain=mesh, '
                'subdomain_data=markers)' % (measure, subdomain_id, measure))
    elif markers.mesh is not mesh:
        raise ValueError('the facet markers belong to another mesh')


def _check_cell_markers(mesh, markers, subdomain_id):
    if markers is None:
        raise ValueError('dx(%r) needs markers: Measure(\'dx\', domain=mesh, '
                         'subdomain_data=markers)' % (subdomain_id,))
    if markers.mesh is not mesh:
        raise ValueError('the cell markers belong to another mesh')
    if getattr(markers, 'dim', None) != 2:
        raise ValueError('dx(%r) takes a cell MeshFunction (dim 2) as '
                         'subdomain_data' % (subdomain_id,))


# -- host selections -----------------------------------------------------------
def _facet_selection(mesh, markers, subdomain_id):
    '''Positions in mesh.bfacets of the facets ds(subdomain_id) selects.'''
    if subdomain_id in (None, 'everywhere'):
        return numpy.arange(len(mesh.bfacets))
    return numpy.nonzero(markers.array()[mesh.bfacets] == subdomain_id)[0]


def _interior_facet_selection(mesh, markers, subdomain_id):
    '''Positions in Mesh.interior_facet_lists()['facets'] of the facets
    dS(subdomain_id) selects.'''
    facets = mesh.interior_facet_lists()['facets']
    if subdomain_id in (None, 'everywhere'):
        return numpy.arange(len(facets))
    return numpy.nonzero(markers.array()[facets] == subdomain_id)[0]


def _cell_selection(mesh, markers, subdomain_id):
    '''The cells dx(subdomain_id) selects, ascending.'''
    if subdomain_id in (None, 'everywhere'):
        return numpy.arange(mesh.num_cells())
    return numpy.nonzero(markers.array() == subdomain_id)[0]


# -- the cache rule ------------------------------------------------------------
_DEVICE = [None, None]      # the device last seen, and its name


def held(cache, markers, subdomain_id, extra, keep, build, *args):
    '''The value build(*args) of one selection, held in the dict `cache` --
    the SAME object while the entry holds.  An entry is keyed by the markers
    (their id), the subdomain id, `extra` (hashable: rank, cell or facet),
    the id of `keep` and the name of the device; it holds while the markers
    are the same object at the same `version` and `keep` (a layout, or None)
    is the same object.  Markers and `keep` are kept alive with the entry:
    their ids stay unique.  subdomain_id 'everywhere' | None selects without
    markers: none in the key, no version.  A dict that holds 32 entries is
    emptied before the next one goes in.  A time loop therefore uploads
    nothing, and re-marking (MeshFunction bumps its version) rebuilds.'''
    if subdomain_id in (None, 'everywhere'):
        markers = subdomain_id = version = None
    else:
        version = markers.version
    dev = device.get()
    if dev is not _DEVICE[0]:
        _DEVICE[:] = dev, str(dev)
    key = (id(markers), subdomain_id, extra, id(keep), _DEVICE[1])
    entry = cache.get(key)
    if entry is not None and entry[0] is markers and entry[1] == version \
            and entry[2] is keep:
        return entry[3]
    value = build(*args)
    if len(cache) >= 32:
        cache.clear()
    cache[key] = (markers, version, keep, value)
    return value


# -- lists ---------------------------------------------------------------------
def _upload_facet_lists(mesh, markers, subdomain_id):
    sel = _facet_selection(mesh, markers, subdomain_id)
    cells = mesh.bfacet_cell[sel].astype(numpy.int32)
    local = mesh.bfacet_local[sel].astype(numpy.int32)
    if len(sel) == 0:
        return None, None, 0
    return device.to_device(cells), device.to_device(local), len(sel)


def facet_lists(mesh, markers=None, subdomain_id='everywhere'):
    '''The exterior facets a ds integral runs over, as device int32 arrays
    (owning cell, local facet index) and their count: every boundary facet
    for subdomain_id 'everywhere', else those whose marker equals
    subdomain_id, in boundary-facet order.  Cached on the mesh against the
    markers' version: a time loop uploads nothing, re-marking re-selects.'''
    _check_facet_markers(mesh, markers, subdomain_id)
    return held(mesh._cache.setdefault('facet_lists', {}), markers,
                subdomain_id, None, None, _upload_facet_lists, mesh, markers,
                subdomain_id)


InteriorFacetLists = collections.namedtuple(
    'InteriorFacetLists', 'plus local other count positions cell_positions')


def _upload_interior_facet_lists(mesh, markers, subdomain_id):
    lists = mesh.interior_facet_lists()
    sel = _interior_facet_selection(mesh, markers, subdomain_id)
    count = len(sel)
    positions = numpy.full(mesh.num_edges(), -1, dtype=numpy.int32)
    positions[lists['facets'][sel]] = numpy.arange(count, dtype=numpy.int32)
    plus = local = other = cellpos = None
    if count:
        nc = mesh.num_cells()
        if nc >= 1 << 28:
            raise ValueError('the interior facet list packs cell indices '
                             'below 2**28; the mesh has %d cells' % nc)
        packed = (lists['cell_minus'][sel].astype(numpy.int64) << 3) \
            | (lists['local_minus'][sel].astype(numpy.int64) << 1) \
            | lists['flip'][sel]
        plus = device.to_device(lists['cell_plus'][sel].astype(numpy.int32))
        local = device.to_device(lists['local_plus'][sel].astype(numpy.int32))
        other = device.to_device(packed.astype(numpy.int32))
        cellpos = device.to_device(numpy.ascontiguousarray(
            positions[mesh.cell_edges].T.reshape(-1)))
    return InteriorFacetLists(plus, local, other, count, positions, cellpos)


def interior_facet_lists(mesh, markers=None, subdomain_id='everywhere'):
    '''The interior facets a dS integral runs over: device int32 arrays
    `plus`, `local` (the '+' cell -- the smaller cell index -- and the
    facet's local index in it) and `other` ((cell- << 3) | (local- << 1) |
    flip, as adapt.facet_table packs a neighbour), their `count`, and for the
    cell gather `positions` (host, one entry per EDGE of the mesh: the
    facet's place in the selection or -1) and `cell_positions` (device
    (3*nc,): entry [i*nc + c] = positions[cell_edges[c][i]]).  Every interior
    facet for subdomain_id 'everywhere', else those whose marker equals
    subdomain_id, in Mesh.interior_facets order.  Cached on the mesh against
    the markers' version like facet_lists; an empty selection holds no device
    array.'''
    _check_facet_markers(mesh, markers, subdomain_id, 'dS')
    return held(mesh._cache.setdefault('interior_facet_lists', {}), markers,
                subdomain_id, None, None, _upload_interior_facet_lists, mesh,
                markers, subdomain_id)


def _upload_cell_list(mesh, markers, subdomain_id):
    sel = _cell_selection(mesh, markers, subdomain_id)
    if len(sel) == 0:
        return None, 0
    return device.to_device(sel.astype(numpy.int32)), len(sel)


def cell_lists(mesh, markers=None, subdomain_id='everywhere'):
    '''The cells a dx(k) integral runs over: a device int32 array of the
    cells whose marker equals subdomain_id, ascending, and their count.
    Cached on the mesh against the markers' version like facet_lists: a time
    loop uploads nothing, re-marking re-selects.  An empty selection holds no
    device array; for 'everywhere' nothing is built, (None, number of cells)
    -- the whole-mesh entry points take no list.'''
    if subdomain_id in (None, 'everywhere'):
        return None, mesh.num_cells()
    _check_cell_markers(mesh, markers, subdomain_id)
    return held(mesh._cache.setdefault('cell_lists', {}), markers,
                subdomain_id, None, None, _upload_cell_list, mesh, markers,
                subdomain_id)


# -- contribution maps ---------------------------------------------------------
def by_target(tgt, n):
    '''(targets, ptr, src), numpy int32, of the scratch of a list launch over
    n items: tgt[s] (int64) is where scratch entry s = ij*n + k -- element
    entry ij of item k of the list -- is added.  targets: the sorted unique
    values of tgt; target t sums scratch[src[e]], e in [ptr[t], ptr[t+1]),
    ascending by the item's position k, then by ij.  Every scratch entry
    appears exactly once.  n = 0: no target, ptr [0].'''
    if n == 0:
        return (numpy.zeros(0, numpy.int32), numpy.zeros(1, numpy.int32),
                numpy.zeros(0, numpy.int32))
    assert len(tgt) < 2**31
    scr = numpy.arange(len(tgt), dtype=numpy.int64)
    order = numpy.lexsort((scr // n, scr % n, tgt))     # (target, k, ij)
    st = tgt[order]
    first = numpy.nonzero(numpy.concatenate([[True], st[1:] != st[:-1]]))[0]
    return (st[first].astype(numpy.int32),
            numpy.concatenate([first, [len(st)]]).astype(numpy.int32),
            order.astype(numpy.int32))


def facet_map_host(mesh, layout, rank, markers=None,
                   subdomain_id='everywhere'):
    '''The facet contribution map of one (facet selection, space layout) pair
    as numpy int32 arrays (targets, ptr, src).  The lanes of
    flow_form_facet_matrix / flow_form_facet_vector write the element entries
    of facet k of the selection (facet_lists' order) to scratch[(i*NL + j)*nf
    + k] (rank 2) or scratch[i*nf + k] (rank 1), NL = layout.nloc -- ALL the
    dofs of the owning cell, not only those on the edge.  targets: the sorted
    unique indices of the nonzeros of the layout's CSR pattern (rank 2) or of
    the dofs (rank 1) that any listed facet's cell touches; target t sums
    scratch[src[e]], e in [ptr[t], ptr[t+1]), ascending by facet position,
    then by ij (i).  Every scratch entry appears exactly once.'''
    sel = _facet_selection(mesh, markers, subdomain_id)
    if len(sel) == 0:
        return by_target(None, 0)
    cd = layout.cell_dofs[mesh.bfacet_cell[sel]].astype(numpy.int64)  # (nf, nl)
    if rank == 1:
        tgt = cd.T.reshape(-1)                          # [i][k]
    else:
        N = layout.N
        key = (cd[:, :, None] * N + cd[:, None, :]).transpose(1, 2, 0)
        key = key.reshape(-1)                           # [i*nl + j][k]
        rowptr = layout.pattern('rowptr').astype(numpy.int64)
        ukey = numpy.repeat(numpy.arange(N, dtype=numpy.int64),
                            numpy.diff(rowptr)) * N + layout.pattern('cols')
        tgt = numpy.searchsorted(ukey, key)
        assert (ukey[tgt] == key).all()
    return by_target(tgt, len(sel))


def cell_map_host(mesh, layout, rank, markers=None, subdomain_id='everywhere'):
    '''The cell contribution map of one (cell selection, space layout, rank)
    as numpy int32 arrays (targets, ptr, src), of the shape of facet_map_host.
    The lanes of flow_form_cells_matrix / flow_form_cells_vector write the
    element entries of cell k of the selection (cell_lists' order) to
    scratch[(i*NL + j)*nsel + k] (rank 2) or scratch[i*nsel + k] (rank 1), NL
    = layout.nloc.  targets: the sorted unique indices of the nonzeros of the
    layout's CSR pattern (rank 2) or of the dofs (rank 1) that a selected
    cell touches; target t sums scratch[src[e]], e in [ptr[t], ptr[t+1]).
    ORDER: the sources of a target stand in the order in which the space's
    own map lists them (cptr / csrc, rank 2; vptr / vsrc, rank 1), restricted
    to the selected cells -- the space's map is filtered: the cell of each
    source is decoded, unselected cells are dropped, the rest re-encoded with
    the cell's position in the list.  A selection that holds every cell
    therefore gives the bits of plain dx.  Every scratch entry appears exactly
    once.'''
    sel = _cell_selection(mesh, markers, subdomain_id)
    nsel, nc = len(sel), mesh.num_cells()
    if nsel == 0:
        return by_target(None, 0)
    if rank == 2:
        ptr, src = layout.pattern('cptr'), layout.pattern('csrc')
    else:
        ptr, src = layout.vmap('vptr'), layout.vmap('vsrc')
    src = src.astype(numpy.int64)
    position = numpy.full(nc, -1, dtype=numpy.int64)
    position[sel] = numpy.arange(nsel)
    pos = position[src % nc]
    keep = pos >= 0
    # (kept sources before each row of the space's map: the new row pointers)
    before = numpy.concatenate([[0], numpy.cumsum(keep)])[ptr]
    count = numpy.diff(before)
    targets = numpy.nonzero(count)[0]
    new_src = (src[keep] // nc) * nsel + pos[keep]
    assert len(new_src) == layout.nloc**rank * nsel < 2**31
    return (targets.astype(numpy.int32),
            numpy.concatenate([before[targets], [len(new_src)]]).astype(
                numpy.int32),
            new_src.astype(numpy.int32))


def device_map(host_triple):
    '''A host map (targets, ptr, src) on the device: (targets, ptr, src,
    number of targets); (None, None, None, 0) for an empty map.'''
    targets, ptr, src = host_triple
    if len(targets) == 0:
        return None, None, None, 0
    return (device.to_device(targets), device.to_device(ptr),
            device.to_device(src), len(targets))


def _upload_map(host_map, *args):
    return device_map(host_map(*args))


def facet_map(mesh, layout, rank, markers=None, subdomain_id='everywhere'):
    '''facet_map_host on the device: (targets, ptr, src, number of targets),
    None arrays for an empty selection.  Cached on the mesh next to the
    facet_lists entry and against the markers' version in the same way: a time
    loop uploads nothing, re-marking rebuilds.  The SAME tuple is returned
    while the entry holds.'''
    _check_facet_markers(mesh, markers, subdomain_id)
    return held(mesh._cache.setdefault('facet_maps', {}), markers,
                subdomain_id, rank, layout, _upload_map, facet_map_host, mesh,
                layout, rank, markers, subdomain_id)


def cell_map(mesh, layout, rank, markers=None, subdomain_id='everywhere'):
    '''cell_map_host on the device: (targets, ptr, src, number of targets),
    None arrays for an empty selection.  Cached on the mesh against the
    markers' version like facet_map; the SAME tuple is returned while the
    entry holds.'''
    _check_cell_markers(mesh, markers, subdomain_id)
    return held(mesh._cache.setdefault('cell_maps', {}), markers,
                subdomain_id, rank, layout, _upload_map, cell_map_host, mesh,
                layout, rank, markers, subdomain_id)


def rect_map(R, cell, markers=None, subdomain_id='everywhere'):
    '''The contribution map of a ds (`cell` False) or dx(k) (True) selection
    over the rectangular pattern R (space.RectLayout) on the device:
    R.facet_map_host | R.cell_map_host as (targets, ptr, src, number of
    targets), held on R itself (R._dev['maps']) like facet_map.'''
    if cell:
        _check_cell_markers(R.mesh, markers, subdomain_id)
    else:
        _check_facet_markers(R.mesh, markers, subdomain_id)
    return held(R._dev.setdefault('maps', {}), markers, subdomain_id, cell,
                None, _upload_map,
                R.cell_map_host if cell else R.facet_map_host, markers,
                subdomain_id)
