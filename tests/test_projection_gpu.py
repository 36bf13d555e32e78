# -*- coding: utf-8 -*-
'''
fem.Projection on the HIP path (flow_amd/fem/projection.py; csrc/
projection_kernels.hip) against the numpy restatement of tests/
projection_reference.py, on the mesh pairs named there.  That the
restatement alone meets every condition below is checked on the CPU by
tests/test_projection_host.py.

Bounds.  Coverage: 1e-12 (sums of a handful of clipped areas, each good to
a few ulp of the cell's area).  Load vector: entrywise 1e-12 relative to
max|b|, the bound of the form tests for the same kind of per-cell quadrature
sums.  Conservation: 1e-11 relative.  Reproduction: 1e-10 at every dof -- the
margin over the load bound is the mass matrix's condition number (~10 for
these quasi-uniform meshes, up to ~100 for the refined one) times the
solver's rtol = 1e-12.

Every test prints what it measured next to its bound (pytest -s).
'''
import functools

import numpy
import pytest
import torch

from flow_amd import device, fem
from flow_amd.fem import Projection, Transfer, projection

import projection_reference as pref

pytestmark = pytest.mark.gpu

LOAD_BOUND = 1.0e-12
NAMES = sorted(pref.PAIRS)


def _lin(x, y):
    return 3.0 + x - 2.0 * y


def _lin2(x, y):
    return -1.0 + 0.25 * x + 4.0 * y


def _quad(x, y):
    return 1.0 + 2.0 * x - 3.0 * y + 0.5 * x * x + x * y - 2.0 * y * y


def _quad2(x, y):
    return -0.5 + x - y + 3.0 * x * x - 2.0 * x * y + y * y


def _wave(x, y):
    return numpy.sin(5 * x) * numpy.cos(3 * y) + 1.5


def _wave2(x, y):
    return numpy.exp(x - y) * numpy.cos(4 * x * y) - 0.25


def gaussian(x, y):
    return numpy.exp(-((x - 0.27)**2 + (y - 0.31)**2) / (2 * 0.05**2))


@functools.lru_cache(maxsize=None)
def _space(mesh, deg, dim):
    return fem.FunctionSpace(mesh, 'CG', deg, dim=dim)


def _function(V, values):
    u = fem.Function(V)
    u.set_array(values)
    return u


@functools.lru_cache(maxsize=None)
def _projection(name, deg_from, deg_to, dim):
    mesh_from, mesh_to, _ = pref.pair(name)
    return Projection(_space(mesh_from, deg_from, dim), _space(mesh_to, deg_to, dim),
                      allow_partial=(name == 'partial'))


def _integrals(w):
    '''fem.integral of every component of w.'''
    V = w.function_space()
    S = _space(V.mesh(), V.degree, 1)
    return numpy.array([fem.integral(fem.Function(S, w.data[a * V.N:(a + 1) * V.N]))
                        for a in range(V.dim)])


# -- coverage -----------------------------------------------------------------------
@pytest.mark.parametrize('name', pref.COVERED)
def test_coverage_is_one(hip, name):
    mesh_from, mesh_to, sm = pref.pair(name)
    P = _projection(name, 1, 1, 1)
    cov = device.to_host(P.coverage).numpy()
    assert cov.shape == (mesh_to.num_cells(),)
    err = numpy.abs(cov - 1.0).max()
    print('%s: |coverage - 1| %.2e  bound 1e-12  pairs %d' % (name, err, P.pairs))
    assert err <= 1e-12
    assert P.min_coverage == cov.min()
    assert P.pairs == len(projection.pair_list(mesh_from, mesh_to)[1])


def test_partial_coverage(hip):
    mesh_from, mesh_to, sm = pref.pair('partial')
    V_from, V_to = _space(mesh_from, 1, 1), _space(mesh_to, 1, 1)
    part = int((sm.coverage < projection.FULL).sum())
    with pytest.raises(ValueError, match='%d of %d target cells' % (
            part, mesh_to.num_cells())) as info:
        Projection(V_from, V_to)
    assert repr(float(sm.coverage.min()))[:12] in str(info.value)
    P = _projection('partial', 1, 1, 1)
    cov = device.to_host(P.coverage).numpy()
    # no cell is left out: the reference has no sliver below 1e-9
    assert not (sm.coverage < 1e-9).any()
    err = numpy.abs(cov - sm.coverage).max()
    print('partial: coverage error %.2e  bound 1e-12  min %.15f'
          % (err, P.min_coverage))
    assert err <= 1e-12
    assert abs(P.min_coverage - sm.coverage.min()) <= 1e-12
    assert P.min_coverage == cov.min()


def test_uncovered_cell_is_refused(hip):
    src = fem.UnitSquareMesh(3, 3)
    dst = fem.RectangleMesh(fem.Point(0.5, 0.5), fem.Point(2.0, 2.0), 3, 3)
    for allow in (False, True):
        with pytest.raises(ValueError, match='target cells'):
            Projection(_space(src, 1, 1), _space(dst, 1, 1), allow_partial=allow)


# -- the load vector ------------------------------------------------------------------
@pytest.mark.parametrize('dim', [1, 2])
@pytest.mark.parametrize('deg_to', [1, 2])
@pytest.mark.parametrize('deg_from', [1, 2])
@pytest.mark.parametrize('name', NAMES)
def test_load_vector(hip, name, deg_from, deg_to, dim):
    _, _, sm = pref.pair(name)
    P = _projection(name, deg_from, deg_to, dim)
    values = pref.nodal(P.V_from, (_wave, _wave2)[:dim])
    want = sm.load(P.V_from, P.V_to, values, scale=(name == 'partial'))
    b = P.load(_function(P.V_from, values))
    assert b.shape == (P.V_to.size(),) and b.is_cuda
    got = device.to_host(b).numpy()
    err = numpy.abs(got - want).max() / numpy.abs(want).max()
    print('%s P%d -> P%d dim %d: load error %.2e  bound %.0e'
          % (name, deg_from, deg_to, dim, err, LOAD_BOUND))
    assert err <= LOAD_BOUND


# -- conservation ---------------------------------------------------------------------
@pytest.mark.parametrize('dim', [1, 2])
@pytest.mark.parametrize('deg_to', [1, 2])
@pytest.mark.parametrize('deg_from', [1, 2])
@pytest.mark.parametrize('name', ['non_nested', 'coarse_to_fine',
                                  'fine_to_coarse', 'many'])
def test_integral_is_kept(hip, name, deg_from, deg_to, dim):
    P = _projection(name, deg_from, deg_to, dim)
    u = _function(P.V_from, pref.nodal(P.V_from, (_wave, _wave2)[:dim]))
    w = P.apply(u)
    assert w.function_space().same_as(P.V_to)
    want, got = _integrals(u), _integrals(w)
    err = numpy.abs(got - want) / numpy.abs(want)
    print('%s P%d -> P%d dim %d: integral error %s  bound 1e-11'
          % (name, deg_from, deg_to, dim, err))
    assert (err <= 1e-11).all()


@pytest.mark.parametrize('deg', [1, 2])
def test_interpolation_loses_what_projection_keeps(hip, deg):
    '''Fine -> coarse, a narrow Gaussian: Transfer's integral error is at
    least 100 x the projection's.'''
    P = _projection('fine_to_coarse', deg, deg, 1)
    u = _function(P.V_from, pref.nodal(P.V_from, (gaussian,)))
    want = fem.integral(u)
    proj = abs(fem.integral(P.apply(u)) - want)
    interp = abs(fem.integral(Transfer(P.V_from, P.V_to).apply(u)) - want)
    print('P%d: integral %.6e  projection error %.2e  interpolation error %.2e'
          % (deg, want, proj, interp))
    assert proj <= 1e-11 * abs(want)
    assert interp >= 100.0 * proj and interp >= 1e-3 * abs(want)


# -- reproduction ---------------------------------------------------------------------
@pytest.mark.parametrize('dim', [1, 2])
@pytest.mark.parametrize('name', pref.COVERED)
def test_polynomials_come_back(hip, name, dim):
    for deg, funcs in ((1, (_lin, _lin2)), (2, (_quad, _quad2))):
        P = _projection(name, deg, deg, dim)
        w = P.apply(_function(P.V_from, pref.nodal(P.V_from, funcs[:dim])))
        err = numpy.abs(w.array() - pref.nodal(P.V_to, funcs[:dim])).max()
        print('%s P%d dim %d: reproduction error %.2e  bound 1e-10'
              % (name, deg, dim, err))
        assert err <= 1e-10


@pytest.mark.parametrize('dim', [1, 2])
@pytest.mark.parametrize('deg', [1, 2])
def test_same_space_is_the_identity(hip, deg, dim):
    P = _projection('same', deg, deg, dim)
    values = pref.nodal(P.V_from, (_wave, _wave2)[:dim])
    w = P.apply(_function(P.V_from, values))
    err = numpy.abs(w.array() - values).max()
    print('P%d dim %d: |P u - u| %.2e  bound 1e-10' % (deg, dim, err))
    assert err <= 1e-10


@pytest.mark.parametrize('name', pref.COVERED)
def test_quadratic_into_p1_against_dense_solve(hip, name):
    _, _, sm = pref.pair(name)
    P = _projection(name, 2, 1, 2)
    values = pref.nodal(P.V_from, (_quad, _quad2))
    want = sm.project(P.V_from, P.V_to, values)
    got = P.apply(_function(P.V_from, values)).array()
    err = numpy.abs(got - want).max()
    print('%s P2 -> P1: against the dense solve %.2e  bound 1e-10' % (name, err))
    assert err <= 1e-10


def test_project_onto_and_out(hip):
    P = _projection('non_nested', 2, 1, 1)
    u = _function(P.V_from, pref.nodal(P.V_from, (_wave,)))
    want = P.apply(u)
    assert torch.equal(fem.project_onto(u, P.V_to).data, want.data)
    w = _function(P.V_to, numpy.full(P.V_to.size(), 7.0))   # not a start vector
    ptr = w.data.data_ptr()
    assert P.apply(u, out=w) is w and w.data.data_ptr() == ptr
    assert torch.equal(w.data, want.data)


# -- determinism ------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['many', 'partial'])
def test_two_calls_give_the_same_bits(hip, name):
    P = _projection(name, 2, 2, 2)
    u = _function(P.V_from, pref.nodal(P.V_from, (_wave, _wave2)))
    assert torch.equal(P.load(u), P.load(u))
    assert torch.equal(P.apply(u).data, P.apply(u).data)


# -- robustness -------------------------------------------------------------------------
def test_nothing_is_written_past_the_results(hip):
    from flow_amd import _hip
    from flow_amd.fem import ops
    mesh_from, mesh_to, _ = pref.pair('many')
    V_from, V_to = _space(mesh_from, 1, 2), _space(mesh_to, 2, 2)
    P = Projection(V_from, V_to)
    nc, used = P.nc, 2 * 6 * P.nc
    buf = ops.scratch(mesh_to, used + 512)
    _hip.fill(buf, float('nan'))
    cov = _hip.fill(device.empty(nc + 64), float('nan'))
    P.coverage = cov[:nc]
    b = P.load(_function(V_from, pref.nodal(V_from, (_wave, _wave2))))
    assert ops.scratch(mesh_to, used).data_ptr() == buf.data_ptr()
    assert torch.isfinite(b).all()
    assert torch.isfinite(buf[:used]).all() and torch.isnan(buf[used:]).all()
    assert torch.isfinite(cov[:nc]).all() and torch.isnan(cov[nc:]).all()


def test_bad_pair_list_gives_nan_in_that_cell(hip):
    '''A guarded read: source indices outside the source mesh put NaN into
    the dofs of their target cells and into their coverage, nothing else.'''
    mesh_from, mesh_to, _ = pref.pair('non_nested')
    V_from, V_to = _space(mesh_from, 2, 1), _space(mesh_to, 2, 1)
    P = Projection(V_from, V_to)
    u = _function(V_from, pref.nodal(V_from, (_wave,)))
    good = device.to_host(P.load(u)).numpy().copy()
    pptr, psrc = projection.pair_list(mesh_from, mesh_to)
    bad = psrc.copy()
    cells = (3, mesh_to.num_cells() - 1)
    bad[pptr[cells[0]]] = mesh_from.num_cells()            # one past the end
    bad[pptr[cells[1] + 1] - 1] = -1
    b = torch.empty(V_to.size(), dtype=torch.float64, device=device.get())
    got = device.to_host(P._load(u, b, psrc=device.to_device(bad))).numpy()
    hit = numpy.zeros(V_to.N, dtype=bool)
    hit[V_to.layout.cell_dofs[list(cells)].ravel()] = True
    assert numpy.isnan(got[hit]).all()
    assert numpy.array_equal(got[~hit], good[~hit])
    cov = device.to_host(P.coverage).numpy()
    assert numpy.isnan(cov[list(cells)]).all()
    assert numpy.isfinite(numpy.delete(cov, cells)).all()
