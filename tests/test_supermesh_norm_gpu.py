# -*- coding: utf-8 -*-
'''
fem.Supermesh on the HIP path (flow_amd/fem/supermesh.py; csrc/
projection_kernels.hip: flow_supermesh_norms) against the numpy restatement
of tests/supermesh_norm_reference.py, on the mesh pairs of the projection
tests.  That the restatement alone meets the analytic values is checked on
the CPU by tests/test_supermesh_norm_host.py.

Bounds.  1e-12 throughout, the bound of the form and projection tests for the
same clipping and quadrature arithmetic: per-cell values relative to the
largest cell value, norms and products relative to themselves, coverage and
area absolute (they are of order 1).  The sums are compared to the last bit
with the restatement of the device's order of summation.

Every test prints what it measured next to its bound (pytest -s).
'''
import ctypes
import functools
import math

import numpy
import pytest
import torch

from flow_amd import _hip, device, fem
from flow_amd.fem import Supermesh, Transfer, assemble, dx, grad, inner, projection
from flow_amd.fem import ops

import supermesh_norm_reference as sref

pytestmark = pytest.mark.gpu

BOUND = 1.0e-12
NAMES = sorted(sref.PAIRS)
DEGREES = [(1, 1), (1, 2), (2, 1), (2, 2)]
NORMS = ('L2', 'H10', 'H1')


def _x(x, y):
    return x + 0.0 * y


def _y(x, y):
    return y + 0.0 * x


def _wave(x, y):
    return numpy.sin(5 * x) * numpy.cos(3 * y) + 1.5


def _wave2(x, y):
    return numpy.exp(x - y) * numpy.cos(4 * x * y) - 0.25


def _other(x, y):
    return numpy.cos(4 * x + 1.0) * numpy.sin(2 * y) + 1.25 + 0.5 * x


def _other2(x, y):
    return numpy.exp(0.5 * y - x) * numpy.sin(3 * x * y + 0.3) + 0.5


@functools.lru_cache(maxsize=None)
def _space(mesh, deg, dim):
    return fem.FunctionSpace(mesh, 'CG', deg, dim=dim)


def _function(V, funcs):
    u = fem.Function(V)
    u.set_array(sref.pref.nodal(V, funcs[:V.dim]))
    return u


@functools.lru_cache(maxsize=None)
def _supermesh(name, deg_a, deg_b, dim):
    mesh_a, mesh_b, _ = sref.pair(name)
    return Supermesh(_space(mesh_a, deg_a, dim), _space(mesh_b, deg_b, dim),
                     allow_partial=(name == 'partial'))


@functools.lru_cache(maxsize=None)
def _case(name, deg_a, deg_b, dim):
    '''(S, u, w, the restatement's result) with smooth non-polynomial nodal
    data: computed once, shared and left unchanged.'''
    S = _supermesh(name, deg_a, deg_b, dim)
    u = _function(S.V_a, (_wave, _wave2))
    w = _function(S.V_b, (_other, _other2))
    return S, u, w, sref.norms(name, S.V_a, S.V_b, u.array(), w.array())


def _rel(a, b):
    return abs(a - b) / abs(b)


def _host(t):
    return device.to_host(t).numpy().copy()


def _bits(x):
    return numpy.float64(x).view(numpy.int64)


# -- the values per cell ----------------------------------------------------------------
@pytest.mark.parametrize('dim', [1, 2])
@pytest.mark.parametrize('deg_a,deg_b', DEGREES)
@pytest.mark.parametrize('name', NAMES)
def test_cell_errors_against_the_restatement(hip, name, deg_a, deg_b, dim):
    S, u, w, want = _case(name, deg_a, deg_b, dim)
    nc = S.V_b.mesh().num_cells()
    got = {}
    for k in NORMS:
        t = S.cell_errors(u, w, k)
        assert t.shape == (nc,) and t.is_cuda and t.dtype == torch.float64
        assert t.is_contiguous()
        got[k] = _host(t)
    err = {k: numpy.abs(got[k] - want[r]).max() / numpy.abs(want[r]).max()
           for k, r in (('L2', 'l2'), ('H10', 'h10'))}
    values, _ = S._cell_values(u, w, product=True)
    prod = _host(values).reshape(2, nc)
    err['uw'] = numpy.abs(prod[0] - want['uw']).max() / numpy.abs(want['uw']).max()
    err['gugw'] = numpy.abs(prod[1] - want['gugw']).max() \
        / numpy.abs(want['gugw']).max()
    print('%s P%d, P%d dim %d: cell L2 %.2e  H10 %.2e  u w %.2e  gu.gw %.2e  '
          'bound %.0e' % (name, deg_a, deg_b, dim, err['L2'], err['H10'],
                          err['uw'], err['gugw'], BOUND))
    assert max(err.values()) <= BOUND
    assert numpy.array_equal(got['H1'], got['L2'] + got['H10'])
    assert (got['L2'] >= 0.0).all() and (got['H10'] >= 0.0).all()


@pytest.mark.parametrize('name', NAMES)
def test_coverage_and_area(hip, name):
    mesh_a, mesh_b, sm = sref.pair(name)
    S = _supermesh(name, 1, 1, 1)
    cov = _host(S.coverage)
    assert cov.shape == (mesh_b.num_cells(),)
    area = float(sm.area.sum())
    e_cov, e_area = numpy.abs(cov - sm.coverage).max(), abs(S.area - area)
    print('%s: coverage %.2e  area %.2e (%.15f)  bound %.0e  pairs %d'
          % (name, e_cov, e_area, S.area, BOUND, S.pairs))
    assert e_cov <= BOUND and e_area <= BOUND
    assert isinstance(S.area, float) and S.min_coverage == cov.min()
    assert S.pairs == len(projection.pair_list(mesh_a, mesh_b)[1])
    if name in sref.COVERED:
        assert abs(S.area - 1.0) <= BOUND


def test_partial_coverage(hip):
    '''Refused without allow_partial, with the count of partly covered cells
    and the worst coverage; with it the integrals over the overlap (the
    values: the cases named `partial` above).'''
    mesh_a, mesh_b, sm = sref.pair('partial')
    V_a, V_b = _space(mesh_a, 1, 1), _space(mesh_b, 1, 1)
    part = int((sm.coverage < projection.FULL).sum())
    assert part >= 10
    with pytest.raises(ValueError, match='%d of %d target cells' % (
            part, mesh_b.num_cells())) as info:
        Supermesh(V_a, V_b)
    assert repr(float(sm.coverage.min()))[:12] in str(info.value)
    with pytest.raises(ValueError, match='%d of %d target cells' % (
            part, mesh_b.num_cells())):
        fem.mesh_errornorm(fem.Function(V_a), fem.Function(V_b))
    S = _supermesh('partial', 1, 1, 1)
    assert abs(S.min_coverage - sm.coverage.min()) <= BOUND
    assert S.area < mesh_b.cell_areas().sum() - 1e-3
    # the area of the overlap is int 1 * 1 over it
    one_a, one_b = _function(V_a, (lambda x, y: 1.0 + 0.0 * x,)), \
        _function(V_b, (lambda x, y: 1.0 + 0.0 * x,))
    got = S.inner(one_a, one_b)
    print('partial: int 1 over the overlap %.15f  area %.15f' % (got, S.area))
    assert _rel(got, S.area) <= BOUND
    assert fem.mesh_errornorm(one_a, one_b, allow_partial=True) <= 1e-12


# -- norms --------------------------------------------------------------------------------
@pytest.mark.parametrize('deg_a,deg_b', DEGREES)
@pytest.mark.parametrize('name', sref.COVERED)
def test_errornorm_of_x_against_y(hip, name, deg_a, deg_b):
    '''On the unit square |x - y|_L2 = sqrt(1/6), |x - y|_H10 = sqrt(2).'''
    S = _supermesh(name, deg_a, deg_b, 1)
    u, w = _function(S.V_a, (_x,)), _function(S.V_b, (_y,))
    l2, h10, h1 = (S.errornorm(u, w, k) for k in NORMS)
    assert S.errornorm(u, w) == l2
    err = (_rel(l2, math.sqrt(1.0 / 6.0)), _rel(h10, math.sqrt(2.0)),
           _rel(h1, math.sqrt(l2**2 + h10**2)))
    print('%s P%d, P%d: L2 %.2e  H10 %.2e  H1 %.2e  bound %.0e'
          % ((name, deg_a, deg_b) + err + (BOUND,)))
    assert max(err) <= BOUND
    assert _rel(S.inner(u, w), 0.25) <= BOUND
    assert abs(S.inner(u, w, 'H10')) <= BOUND
    if (deg_a, deg_b) == (2, 1):
        assert fem.mesh_errornorm(u, w, 'H1') == h1


@pytest.mark.parametrize('dim', [1, 2])
@pytest.mark.parametrize('deg', [1, 2])
def test_error_against_itself_is_zero(hip, deg, dim):
    S = _supermesh('same', deg, deg, dim)
    u = _function(S.V_a, (_wave, _wave2))
    err, norm = S.errornorm(u, u), math.sqrt(S.inner(u, u))
    print('P%d dim %d: |u - u| %.2e  |u| %.3e  bound 1e-12 |u|' % (deg, dim, err, norm))
    assert err <= 1e-12 * norm
    assert _rel(norm, fem.norm(u)) <= BOUND


@pytest.mark.parametrize('dim', [1, 2])
@pytest.mark.parametrize('deg_a,deg_b', DEGREES)
def test_same_mesh_against_assemble(hip, deg_a, deg_b, dim):
    S, u, w, _ = _case('same', deg_a, deg_b, dim)
    d = u - w
    want_l2 = assemble((d**2 if dim == 1 else inner(d, d)) * dx)
    want_h10 = assemble(inner(grad(u), grad(w)) * dx)
    e_l2 = _rel(S.errornorm(u, w)**2, want_l2)
    e_h10 = _rel(S.inner(u, w, 'H10'), want_h10)
    print('same mesh P%d, P%d dim %d: |u - w|^2 %.2e  (grad u, grad w) %.2e  '
          'bound %.0e' % (deg_a, deg_b, dim, e_l2, e_h10, BOUND))
    assert e_l2 <= BOUND and e_h10 <= BOUND


@pytest.mark.parametrize('dim', [1, 2])
@pytest.mark.parametrize('deg', [1, 2])
def test_nested_interpolant_has_no_error(hip, deg, dim):
    '''Coarse -> its refinement, the same degree: Transfer is exact.'''
    S = _supermesh('coarse_to_fine', deg, deg, dim)
    u = _function(S.V_a, (_wave, _wave2))
    w = Transfer(S.V_a, S.V_b).apply(u)
    err, norm = S.errornorm(u, w), fem.norm(u)
    print('nested P%d dim %d: |u - I u| %.2e  |u| %.3e  bound 1e-12 |u|'
          % (deg, dim, err, norm))
    assert err <= 1e-12 * norm


@pytest.mark.parametrize('name', ['non_nested', 'coarse_to_fine', 'partial', 'many'])
def test_inner_does_not_depend_on_the_roles(hip, name):
    S, u, w, _ = _case(name, 2, 1, 2)
    R = Supermesh(S.V_b, S.V_a, allow_partial=(name == 'partial'))
    err = [_rel(R.inner(w, u, k), S.inner(u, w, k)) for k in NORMS]
    print('%s: inner(u, w) against inner(w, u) the other way round %s  bound %.0e'
          % (name, ' '.join('%.2e' % e for e in err), BOUND))
    assert max(err) <= BOUND
    assert abs(R.area - S.area) <= BOUND


# -- the order of summation, determinism ---------------------------------------------------
@pytest.mark.parametrize('name', ['non_nested', 'many', 'partial'])
def test_sums_in_the_stated_order_to_the_last_bit(hip, name):
    '''One block ('non_nested': 30 cells), a full block and 8 lanes of a
    second ('many': 264 cells), 194 cells.'''
    S, u, w, _ = _case(name, 2, 2, 2)
    l2 = sref.sum_in_device_order(_host(S.cell_errors(u, w, 'L2')))
    h10 = sref.sum_in_device_order(_host(S.cell_errors(u, w, 'H10')))
    for k, total in (('L2', l2), ('H10', h10), ('H1', l2 + h10)):
        got = S.errornorm(u, w, k)
        assert _bits(got) == _bits(math.sqrt(total)), (k, got, math.sqrt(total))
    values, totals = S._cell_values(u, w, totals=True)
    assert _bits(totals[0]) == _bits(l2) and _bits(totals[1]) == _bits(h10)
    values, totals = S._cell_values(u, w, product=True, totals=True)
    prod = _host(values).reshape(2, -1)
    uw, gg = (sref.sum_in_device_order(p) for p in prod)
    assert _bits(totals[0]) == _bits(uw) and _bits(totals[1]) == _bits(gg)
    for k, total in (('L2', uw), ('H10', gg), ('H1', uw + gg)):
        assert _bits(S.inner(u, w, k)) == _bits(total)


@pytest.mark.parametrize('name', ['many', 'partial'])
def test_two_calls_give_the_same_bits(hip, name):
    S, u, w, _ = _case(name, 2, 2, 2)
    for k in NORMS:
        assert torch.equal(S.cell_errors(u, w, k), S.cell_errors(u, w, k))
        assert _bits(S.errornorm(u, w, k)) == _bits(S.errornorm(u, w, k))
        assert _bits(S.inner(u, w, k)) == _bits(S.inner(u, w, k))
    out = device.empty(S.nc)
    ptr = out.data_ptr()
    assert S.cell_errors(u, w, 'H1', out=out) is out and out.data_ptr() == ptr
    assert torch.equal(out, S.cell_errors(u, w, 'H1'))
    assert S.cell_errors(u, w, 'H10', out=out) is out
    assert torch.equal(out, S.cell_errors(u, w, 'H10'))


def test_one_launch_and_what_mark_takes(hip):
    S, u, w, _ = _case('many', 2, 2, 2)
    before = _hip.launch_count()
    eta2 = S.cell_errors(u, w)
    assert _hip.launch_count() == before + 1
    mask = fem.mark(eta2, 0.5)
    assert mask.shape == (S.V_b.mesh().num_cells(),) and mask.dtype == bool
    assert 0 < mask.sum() < len(mask)


# -- robustness ---------------------------------------------------------------------------
def test_nothing_is_written_past_the_results(hip):
    S, u, w, _ = _case('many', 1, 2, 2)
    nc = S.nc
    nan = float('nan')
    values = _hip.fill(device.empty(2 * nc + 64), nan)
    work = _hip.fill(device.empty(_hip.REDUCE_WORK + 64), nan)
    got, totals = S._cell_values(u, w, totals=True, values=values, work=work)
    assert got.data_ptr() == values.data_ptr()
    assert torch.isfinite(values[:2 * nc]).all() and torch.isnan(values[2 * nc:]).all()
    assert torch.isnan(work[_hip.REDUCE_WORK:]).all()
    assert math.isfinite(totals[0]) and math.isfinite(totals[1])
    assert _bits(math.sqrt(totals[0])) == _bits(S.errornorm(u, w))


def test_bad_pair_list_gives_nan_in_that_cell(hip):
    '''A guarded read: the entries nc_a and -1 put NaN into both values of
    their target cells and nothing else; they are defined inputs.'''
    S, u, w, _ = _case('non_nested', 2, 2, 1)
    mesh_a, mesh_b, _ = sref.pair('non_nested')
    nc = mesh_b.num_cells()
    good = _host(S._cell_values(u, w)[0]).reshape(2, nc)
    pptr, psrc = projection.pair_list(mesh_a, mesh_b)
    bad = psrc.copy()
    cells = [3, nc - 1]
    bad[pptr[cells[0]]] = mesh_a.num_cells()               # one past the end
    bad[pptr[cells[1] + 1] - 1] = -1
    values, totals = S._cell_values(u, w, totals=True, psrc=device.to_device(bad))
    got = _host(values).reshape(2, nc)
    hit = numpy.zeros(nc, dtype=bool)
    hit[cells] = True
    assert numpy.isnan(got[:, hit]).all()
    assert numpy.isfinite(got[:, ~hit]).all()
    assert numpy.array_equal(got[:, ~hit], good[:, ~hit])
    assert math.isnan(totals[0]) and math.isnan(totals[1])


def test_entry_point_refusals_launch_nothing(hip):
    S, u, w, _ = _case('non_nested', 2, 1, 2)
    V_a, V_b, nc = S.V_a, S.V_b, S.nc
    values = device.empty(2 * nc)
    work = ops.work(_hip.REDUCE_WORK)
    host = (ctypes.c_double * 2)()

    def call(**change):
        a = dict(mesh_a=ctypes.byref(ops.mesh_struct(V_a.mesh())),
                 V_a=ctypes.byref(ops.space_struct(V_a.layout)),
                 mesh_b=ctypes.byref(ops.mesh_struct(V_b.mesh())),
                 V_b=ctypes.byref(ops.space_struct(V_b.layout)), ncomp=2,
                 pptr=_hip.i32(S._pptr), psrc=_hip.i32(S._psrc), npairs=S.pairs,
                 u=_hip.f64(u.data), w=_hip.f64(w.data), product=0,
                 values=_hip.f64(values), work=_hip.f64(work), host=host)
        a.update(change)
        before = _hip.launch_count()
        rc = hip.flow_supermesh_norms(
            a['mesh_a'], a['V_a'], a['mesh_b'], a['V_b'], a['ncomp'], a['pptr'],
            a['psrc'], a['npairs'], a['u'], a['w'], a['product'], a['values'],
            a['work'], a['host'], _hip.stream())
        return rc, _hip.launch_count() - before

    rc, launches = call()
    assert rc == 0 and launches == 4          # the cells, two sums, the read-back
    same = _hip.f64(values)
    for change in (dict(values=None), dict(u=None), dict(w=None), dict(pptr=None),
                   dict(V_a=None), dict(mesh_b=None), dict(work=None),
                   dict(ncomp=3), dict(ncomp=0), dict(product=2),
                   dict(u=same, w=same), dict(u=same), dict(w=same),
                   dict(values=_hip.f64(work)), dict(u=_hip.f64(work))):
        rc, launches = call(**change)
        assert rc == 2 and launches == 0, change
        with pytest.raises(ValueError, match='invalid argument'):
            _hip.check(rc)
