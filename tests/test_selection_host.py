# -*- coding: utf-8 -*-
'''
The one cache rule of flow_amd/fem/selection.py (selection.held), seen through
every cached entry point: the three lists, facet_map, cell_map and the map over
a rectangular pattern that mixed.rect_launch reads (mixed.selection.rect_map,
for facets and for cells).  Host only: device.to_device copies to the CPU.
'''
import gc
import os
import subprocess
import sys
import weakref

import numpy
import pytest

from flow_amd import fem
from flow_amd.fem import MeshFunction, mixed, ops, space

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def on():
    with fem.cell_subdomains(True):
        yield


def _lay(mesh):
    return space.scalar_layout(mesh, 1)


def _rect(mesh):
    return space.rect_layout(mesh, 2, 1)


class Entry(object):
    '''One cached entry point: `call(mesh, markers, id)`, the dict it keeps
    its entries in, the dimension of its markers, its measure's name, and
    `size(value)`, which grows when one more facet | cell is selected.'''

    def __init__(self, call, cache, dim, measure, size):
        self.call, self.cache, self.dim = call, cache, dim
        self.measure, self.size = measure, size


def _src_len(value):
    return 0 if value[2] is None else len(value[2])


ENTRIES = {
    'facet_lists': Entry(
        lambda mesh, m, k: ops.facet_lists(mesh, m, k),
        lambda mesh: mesh._cache['facet_lists'], 1, 'ds', lambda v: v[2]),
    'interior_facet_lists': Entry(
        lambda mesh, m, k: ops.interior_facet_lists(mesh, m, k),
        lambda mesh: mesh._cache['interior_facet_lists'], 1, 'dS',
        lambda v: v.count),
    'cell_lists': Entry(
        lambda mesh, m, k: ops.cell_lists(mesh, m, k),
        lambda mesh: mesh._cache['cell_lists'], 2, 'dx', lambda v: v[1]),
    'facet_map': Entry(
        lambda mesh, m, k: ops.facet_map(mesh, _lay(mesh), 2, m, k),
        lambda mesh: mesh._cache['facet_maps'], 1, 'ds', _src_len),
    'cell_map': Entry(
        lambda mesh, m, k: ops.cell_map(mesh, _lay(mesh), 2, m, k),
        lambda mesh: mesh._cache['cell_maps'], 2, 'dx', _src_len),
    'rect_facet_map': Entry(
        lambda mesh, m, k: mixed.selection.rect_map(_rect(mesh), False, m, k),
        lambda mesh: _rect(mesh)._dev['maps'], 1, 'ds', _src_len),
    'rect_cell_map': Entry(
        lambda mesh, m, k: mixed.selection.rect_map(_rect(mesh), True, m, k),
        lambda mesh: _rect(mesh)._dev['maps'], 2, 'dx', _src_len),
    }
NAMES = sorted(ENTRIES)


def _unselected(mesh, entry):
    '''[two facets | cells the initial marking leaves out], of the kind the
    entry point selects from.'''
    if entry.dim == 2:
        return [0, 2]
    if entry.measure == 'dS':
        return [int(f) for f in mesh.interior_facets[[0, 2]]]
    return [int(f) for f in mesh.bfacets[[0, 2]]]


def _markers(mesh, entry):
    '''Id 1 on a non-trivial subset that leaves _unselected() out.'''
    m = MeshFunction('size_t', mesh, entry.dim, 0)
    mask = numpy.arange(m.size()) % 3 == 1
    mask[_unselected(mesh, entry)] = False
    m.set_where(mask, 1)
    return m


def _same(a, b):
    '''The same object, or a tuple of the same array objects and equal
    counts.'''
    if a is b:
        return True
    return type(a) is tuple and type(b) is tuple and len(a) == len(b) and all(
        x is y or (isinstance(x, int) and x == y) for x, y in zip(a, b))


@pytest.mark.parametrize('name', NAMES)
def test_held_while_the_version_holds(name):
    entry = ENTRIES[name]
    mesh = fem.UnitSquareMesh(4, 3)
    m = _markers(mesh, entry)
    first = entry.call(mesh, m, 1)
    assert entry.size(first) > 0
    assert _same(entry.call(mesh, m, 1), first)
    assert len(entry.cache(mesh)) == 1
    # m[i] = k bumps the version: rebuilt, and one more is selected
    version = m.version
    m[_unselected(mesh, entry)[0]] = 1
    assert m.version == version + 1
    second = entry.call(mesh, m, 1)
    assert not _same(second, first)
    assert entry.size(second) > entry.size(first)
    assert _same(entry.call(mesh, m, 1), second)
    assert len(entry.cache(mesh)) == 1          # (the entry was replaced)
    # markers with equal contents are other markers: an entry of their own
    twin = MeshFunction('size_t', mesh, entry.dim, 0)
    twin.set_where(m.array() == 1, 1)
    assert numpy.array_equal(twin.array(), m.array())
    other = entry.call(mesh, twin, 1)
    assert not _same(other, second)
    assert entry.size(other) == entry.size(second)
    assert len(entry.cache(mesh)) == 2
    assert _same(entry.call(mesh, m, 1), second)
    assert _same(entry.call(mesh, twin, 1), other)


@pytest.mark.parametrize('name', NAMES)
def test_the_entry_keeps_its_markers_alive(name):
    entry = ENTRIES[name]
    mesh = fem.UnitSquareMesh(4, 3)
    m = _markers(mesh, entry)
    entry.call(mesh, m, 1)
    ref = weakref.ref(m)
    del m
    gc.collect()
    assert ref() is not None            # (their id stays unique meanwhile)
    assert _same(entry.call(mesh, ref(), 1), entry.call(mesh, ref(), 1))
    entry.cache(mesh).clear()
    gc.collect()
    assert ref() is None                # (... and nothing else held them)


@pytest.mark.parametrize('name', NAMES)
def test_the_33rd_key_empties_its_own_dict_only(name):
    entry = ENTRIES[name]
    mesh = fem.UnitSquareMesh(4, 3)
    # one entry in the dict of every kind
    keep = {}
    for other, e in ENTRIES.items():
        mo = _markers(mesh, e)
        keep[other] = (mo, e.call(mesh, mo, 1))
    mine = entry.cache(mesh)
    mine.clear()
    m = _markers(mesh, entry)
    for k in range(32):
        entry.call(mesh, m, 100 + k)
        assert len(mine) == k + 1
    before = {other: dict(e.cache(mesh)) for other, e in ENTRIES.items()
              if e.cache(mesh) is not mine}
    assert len(before) >= 5
    entry.call(mesh, m, 132)
    assert len(mine) == 1
    for other, held in before.items():
        e = ENTRIES[other]
        now = e.cache(mesh)
        assert len(held) >= 1 and set(now) == set(held)
        assert all(now[key] is held[key] for key in held)
        mo, value = keep[other]
        assert _same(e.call(mesh, mo, 1), value)


def _message(call, *args):
    with pytest.raises(ValueError) as err:
        call(*args)
    return str(err.value)


@pytest.mark.parametrize('name', NAMES)
def test_refusals_read_the_same_from_every_entry_point(name):
    entry = ENTRIES[name]
    mesh = fem.UnitSquareMesh(4, 3)
    d = entry.measure
    assert _message(entry.call, mesh, None, 3) == (
        "%s(3) needs markers: Measure('%s', domain=mesh, "
        'subdomain_data=markers)' % (d, d))
    elsewhere = MeshFunction('size_t', fem.UnitSquareMesh(2, 2), entry.dim, 0)
    assert _message(entry.call, mesh, elsewhere, 3) == (
        'the %s markers belong to another mesh'
        % ('cell' if entry.dim == 2 else 'facet'))
    if entry.dim == 2:
        facets = MeshFunction('size_t', mesh, 1, 0)
        assert _message(entry.call, mesh, facets, 3) == (
            'dx(3) takes a cell MeshFunction (dim 2) as subdomain_data')
    # nothing was held for a refused call
    assert not any(mesh._cache.get(kind) for kind in (
        'facet_lists', 'interior_facet_lists', 'cell_lists', 'facet_maps',
        'cell_maps'))
    assert not _rect(mesh)._dev.get('maps')


def test_everywhere_takes_no_markers():
    mesh = fem.UnitSquareMesh(4, 3)
    for name in ('facet_lists', 'interior_facet_lists', 'facet_map',
                 'rect_facet_map'):
        entry = ENTRIES[name]
        m = _markers(mesh, entry)
        every = entry.call(mesh, None, 'everywhere')
        assert _same(entry.call(mesh, None, None), every)
        assert _same(entry.call(mesh, m, 'everywhere'), every)
        m[_unselected(mesh, entry)[0]] = 1      # (no version in that key)
        assert _same(entry.call(mesh, m, 'everywhere'), every)
    assert ops.cell_lists(mesh) == (None, mesh.num_cells())
    assert 'cell_lists' not in mesh._cache


def test_selection_does_not_import_ops():
    '''In a fresh interpreter `import flow_amd.fem.selection` imports neither
    ops nor forms nor the library's bindings.  The packages' own __init__
    files import ops for their other modules (stokes, mass, mixed, ...), so
    they are replaced by bare packages over the same directories: what is
    then imported is what selection.py itself asks for.'''
    code = '\n'.join([
        'import os, sys, types',
        'root = sys.argv[1]',
        "for name, path in (('flow_amd', 'flow_amd'),",
        "                   ('flow_amd.fem', 'flow_amd/fem')):",
        '    pkg = types.ModuleType(name)',
        '    pkg.__path__ = [os.path.join(root, path)]',
        '    sys.modules[name] = pkg',
        'import flow_amd.fem.selection as selection',
        "assert selection.__file__.startswith(root), selection.__file__",
        "loaded = sorted(n for n in sys.modules if n.startswith('flow_amd.'))",
        "assert loaded == ['flow_amd.device', 'flow_amd.fem', "
        "'flow_amd.fem.selection'], loaded",
        ])
    subprocess.run([sys.executable, '-c', code, ROOT], check=True, timeout=120)
