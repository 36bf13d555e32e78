# -*- coding: utf-8 -*-
'''
Every launch of the p-multigrid / Chebyshev cycle (flow_pmg_apply,
flow_amd/csrc/pmg_kernels.hip) against an exact model, row by row (-m gpu).

flow_pmg_apply leaves its work buffer behind; runs with different step counts
expose different launches in it (tests/pmg_cycle_reference.py: the model, the
comparator, the inputs; tests/test_pmg_cycle_host.py: that the model is the
textbook cycle and that the comparator can fail).  Real layouts of two small
meshes carry synthetic matrices; the step counts are set in the struct between
applications, the Chebyshev intervals are the ones `refactor` found.  Vector
mode on the whole mesh runs the full grid of (pre, post, coarse_steps); the
int32-column format is held bit for bit against the default one, the one-plane
format, scalar mode and the diagonal blocks of three strips launch by launch.
'''
import functools

import numpy
import pytest

import pmg_cycle_reference as cyc
from fp16_stream_reference import round16

pytestmark = pytest.mark.gpu

MESHES = ('rect', 'karman')


def _dev(a):
    from flow_amd import device
    return device.to_device(numpy.ascontiguousarray(a))


def _host(t):
    from flow_amd import device
    return device.to_host(t).numpy()


def _bits(a):
    a = numpy.ascontiguousarray(a)
    return a.view({2: numpy.uint16, 4: numpy.uint32, 8: numpy.uint64}[
        a.dtype.itemsize])


@functools.lru_cache(maxsize=None)
def _problem(mesh, variant='vector', g=0):
    if variant == 'block':
        return cyc.Problem(mesh, block=(g, 3))
    return cyc.Problem(mesh, one_plane=variant == 'one_plane',
                       scalar=variant == 'scalar')


def _matrix(lay, planes):
    import torch
    from flow_amd import device
    from flow_amd.fem import ops
    J = ops.Matrix(lay, 0 if len(planes) == 1 else 2)
    for i, a in enumerate(planes):
        J.plane(i).copy_(torch.from_numpy(a))
    device.synchronize()
    return J


def _cycle(prob, monkeypatch, cols16=True):
    '''The product's Pmg over the problem's matrices; the problem takes the
    Chebyshev intervals of its structs.'''
    from flow_amd import fem
    from flow_amd.fem import pmg as fpmg
    monkeypatch.setattr(fpmg, 'COLS16', cols16)
    monkeypatch.setattr(fpmg, 'ONE_PLANE', prob.one_plane)
    if prob.scalar:
        W = fem.FunctionSpace(prob.mesh, 'CG', 2)
    else:
        W = fem.VectorFunctionSpace(prob.mesh, 'CG', 2)
    assert W.layout is prob.lay2
    kw = {}
    if prob.block is not None:
        kw = dict(rows=prob.rows, vrows=prob.vrows)
    pre = fpmg.Pmg(W, scalar=prob.scalar, **kw)
    assert (pre.fine.n, pre.coarse.n) == (prob.n, prob.n1)
    for lvl in (pre.fine, pre.coarse):
        assert bool(lvl.struct.cols16) == cols16
        assert bool(lvl.struct.packed) == prob.one_plane
    pre.set_bcs(prob.bc_dofs.astype(numpy.int32))
    pre.refactor(_matrix(prob.lay2, prob.planes),
                 _matrix(prob.lay1, prob.planes1))
    for lvl, L in ((pre.fine, prob.fine), (pre.coarse, prob.coarse)):
        L.lo, L.hi = lvl.struct.lam_min, lvl.struct.lam_max
        assert 0.0 < L.lo < L.hi
    # the tables and masks the device holds are the model's
    k = pre._keep
    assert numpy.array_equal(_host(k['ends']).reshape(-1, 2), prob.ends)
    assert numpy.array_equal(_host(k['rptr']), prob.rptr)
    assert numpy.array_equal(_host(k['rsrc']), prob.rsrc)
    assert numpy.array_equal(cyc.blocked(_host(k['bc_fine']), prob.n), prob.bc)
    assert numpy.array_equal(cyc.blocked(_host(k['bc_coarse']), prob.n1),
                             prob.bcc)
    return pre


def _packed_as_the_model(pre, prob):
    '''What flow_pmg_pack wrote: bit for bit round16 of the (block's) entries,
    zero where a coupling leaves the block; diag and dinv.'''
    for lvl, L, keep in ((pre.fine, prob.fine, prob.keep[0]),
                         (pre.coarse, prob.coarse, prob.keep[1])):
        n, nnz = L.n, L.nnz
        vals = _host(lvl.vals)
        assert numpy.array_equal(_bits(vals[:2 * nnz]).reshape(nnz, 2),
                                 _bits(L.w))
        assert not vals[2 * nnz:].any()
        assert numpy.array_equal(_bits(_host(lvl.diag)).reshape(n, 2),
                                 _bits(L.diag))
        assert numpy.array_equal(_bits(_host(lvl.dinv)).reshape(n, 2),
                                 _bits(L.dinv))
        if keep is not None:
            assert not keep.all() and not L.w[~keep].any()
            assert numpy.array_equal(_host(lvl.keep) != 0, keep)


def _run(pre, prob, cfg, r_dev):
    n, n1 = prob.n, prob.n1
    s = pre.struct
    s.pre, s.post, s.coarse_steps = cfg
    work = pre._keep['work']
    assert work.numel() == cyc.work_size(n, n1)
    assert not _host(work)[-2:].any()           # the dummy slot, before
    z = _dev(numpy.full(2 * n, cyc.SENTINEL))
    pre.apply(r_dev, z)
    return cyc.observe(_host(work), _host(z), n, n1, prob.scalar)


def _compare(pre, prob, configs, tag):
    worst = {}
    for trial in (0, 1):
        r = prob.rhs(trial)
        r_dev = _dev(r)
        runs = dict((cfg, _run(pre, prob, cfg, r_dev)) for cfg in configs)
        for kind, ratio in cyc.compare(prob, r, runs, '%s trial %d' %
                                       (tag, trial)).items():
            worst[kind] = max(ratio, worst.get(kind, 0.0))
    for kind in cyc.KINDS:
        if kind in worst:
            print('RATIO %s %s %.3g' % (tag, kind, worst[kind]))
    return worst


def test_the_meshes_reach_every_path_of_the_restriction():
    lens = numpy.concatenate([_problem(m).list_lengths() for m in MESHES])
    assert (lens < cyc.K_AHEAD).any() and (lens == cyc.K_AHEAD).any() \
        and (lens > cyc.K_AHEAD).any()
    assert max(_problem(m).n for m in MESHES) == 1272


@pytest.mark.parametrize('mesh', MESHES)
def test_every_launch_of_the_grid(hip, mesh, monkeypatch):
    '''Vector mode, whole mesh, 16-bit column offsets: the full grid.'''
    prob = _problem(mesh)
    pre = _cycle(prob, monkeypatch)
    _packed_as_the_model(pre, prob)
    worst = _compare(pre, prob, cyc.GRID, 'pmg ' + mesh)
    assert set(worst) == set(cyc.KINDS)


@pytest.mark.parametrize('mesh', MESHES)
def test_int32_columns_bit_for_bit(hip, mesh, monkeypatch):
    '''COLS16 = False: every work vector and z of (3, 3, 2) as with the 16-bit
    offsets.'''
    prob = _problem(mesh)
    got = {}
    for cols16 in (True, False):
        pre = _cycle(prob, monkeypatch, cols16=cols16)
        got[cols16] = (pre.lam, _run(pre, prob, (3, 3, 2),
                                     _dev(prob.rhs(0))))
    assert got[True][0] == got[False][0]
    a, b = got[True][1], got[False][1]
    for name in sorted(a):
        assert numpy.isfinite(a[name]).all(), name
        assert numpy.array_equal(_bits(a[name]), _bits(b[name])), name
    assert not numpy.array_equal(a['z'], numpy.full_like(a['z'], cyc.SENTINEL))


@pytest.mark.parametrize('mesh', MESHES)
def test_one_plane_launch_by_launch(hip, mesh, monkeypatch):
    prob = _problem(mesh, 'one_plane')
    pre = _cycle(prob, monkeypatch)
    n, n1 = prob.n, prob.n1
    for lvl, L, m in ((pre.fine, prob.fine, n), (pre.coarse, prob.coarse, n1)):
        assert numpy.array_equal(cyc.blocked(_host(lvl._packed[1]), m),
                                 L.idrows)
        assert numpy.array_equal(_bits(_host(lvl.diag)).reshape(m, 2),
                                 _bits(L.diag))
        assert numpy.array_equal(_bits(_host(lvl.dinv)).reshape(m, 2),
                                 _bits(L.dinv))
    _compare(pre, prob, cyc.family(2, 3, 3), 'pmg one_plane ' + mesh)


@pytest.mark.parametrize('mesh', MESHES)
def test_scalar_mode(hip, mesh, monkeypatch):
    '''Pmg(W, scalar=True): lane x == lane y in every work vector, z has n
    entries (the sentinel behind them stays), the NaN behind r is not read
    (the comparator asserts all three).'''
    prob = _problem(mesh, 'scalar')
    assert numpy.isnan(prob.rhs(0)[prob.n:]).all()
    pre = _cycle(prob, monkeypatch)
    _packed_as_the_model(pre, prob)
    _compare(pre, prob, cyc.family(2, 3, 3) + ((1, 1, 1),),
             'pmg scalar ' + mesh)


@pytest.mark.parametrize('g', [0, 1, 2])
def test_block_mode_of_three_strips(hip, g, monkeypatch):
    '''Pmg(W, rows=, vrows=) on the diagonal block of strip g of 3, on one
    GPU: the block pack, local tables, keep-masked weights, the dummy coarse
    row.'''
    prob = _problem('karman', 'block', g)
    # (an edge dof belongs to its lower vertex: the last block has no
    # partner outside)
    assert (prob.ends == prob.n1).any() == (g < 2)
    pre = _cycle(prob, monkeypatch)
    _packed_as_the_model(pre, prob)
    # the block's weights are round16 of the block's own entries
    (r0, r1), lay = prob.rows, prob.lay2
    rp = lay.pattern('rowptr').astype(numpy.int64)
    di = lay.pattern('diag_idx').astype(numpy.int64)
    k0, k1 = int(rp[r0]), int(rp[r1])
    a = prob.planes[0]
    d = numpy.repeat(a[di[r0:r1]], numpy.diff(rp[r0:r1 + 1]))
    want = numpy.where(prob.keep[0], round16(a[k0:k1], d), numpy.float16(0.0))
    assert numpy.array_equal(_bits(prob.fine.w[:, 0]), _bits(want))
    _compare(pre, prob, cyc.family(2, 2, 3), 'pmg block %d' % g)
