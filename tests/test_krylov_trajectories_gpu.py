# -*- coding: utf-8 -*-
'''
Every iterate of flow_cg_solve, flow_cg_solve_guarded, flow_bicgstab_solve and
flow_gmres_solve against textbook solvers in extended precision (-m gpu;
tests/krylov_reference.py, what the comparison can see:
tests/test_krylov_trajectories_host.py).

A solve with maxit = k, rtol = atol = 0 returns FLOW_NOT_CONVERGED with x =
iterate k, *iters_host = k and *resid_host = the norm of that iterate: for
k = 0 .. K, from a fresh start and a workspace full of NaN each time, with
check_every = 1, and once more for k = K with one batch planned past maxit
(first_check / expected_its = K + 5).  The reference runs on the matrices read
back from the device and on the preconditioners as explicit maps of the host
data the product uploads; the tolerance of a case is measured on the host,
reference against reference, before the device is asked (kr.Measured) -- no
figure in this file comes from device output.

Sizes: n = 25 (one workgroup everywhere), n = 841 / 1682 (several, a ragged
last one), n = 263169 > kBlock kRedBlocks and odd (the second grid-stride pass
of cg_update_kernel<true>, gmres_dots_kernel, gmres_combine_dev_kernel).
'''
import ctypes
import functools

import numpy
import pytest

import krylov_reference as kr

pytestmark = pytest.mark.gpu

FLOW_OK, FLOW_NOT_CONVERGED = 0, 1
BIG = (512, 512)          # P1 on a rectangle: 513^2 = 263169 vertices


def _dev(a):
    from flow_amd import device
    return device.to_device(numpy.ascontiguousarray(a))


def _host(t):
    from flow_amd import device
    return device.to_host(t).numpy()


class World(object):
    '''The systems on the device and as host data, the preconditioners on
    both sides, the measured references (built once per module).'''

    def __init__(self):
        from flow_amd import fem
        from flow_amd.fem import ilu, ops
        from flow_amd.fem.multigrid import Multigrid
        p1, lay1 = self._pattern(fem.UnitSquareMesh(4, 4), 1, False)
        p2, lay2 = self._pattern(fem.UnitSquareMesh(10, 10, 'crossed'), 2, True)
        pb, layb = self._pattern(
            fem.RectangleMesh(fem.Point(0.0, 0.0), fem.Point(2.0, 1.0), BIG[0],
                              BIG[1]), 1, False)
        assert lay1.N == 25 and layb.N == 263169 > 256 * 1024
        self.systems = kr.small_systems(p1, p2)
        self.systems['big'] = kr.System(0, pb[0], pb[1], [pb[2]])
        lays = dict(m25=lay1, big=layb)
        self.A, self.dinv = {}, {}
        for name, S in self.systems.items():
            mask = _dev(S.mask) if S.kind == 4 else None
            A = ops.Matrix(lays.get(name, lay2), S.kind,
                           _dev(numpy.concatenate(S.planes)), rowmask=mask)
            assert abs(A.to_scipy() - S.A).max() == 0.0
            self.A[name] = A
            self.dinv[name] = A.diag_inv()
            S.dinv = _host(self.dinv[name])        # (as the device holds it)
        self.vecs = dict((k, kr.starts(k, S)) for k, S in self.systems.items())
        # the preconditioners: device objects and explicit maps
        self.pre = {}
        Ap2 = self.A['p2']
        coarse = ops.CoarseSpace(Ap2, target_nc=30)
        assert coarse.nc % 4 != 0 and coarse.nc > 4, coarse.nc
        A32 = _host(coarse._keep[3])
        self.pre['p2', 'two_level'] = (coarse, lambda dtype: kr.two_level(
            self.systems['p2'].dinv, coarse.agg_of_host, A32, dtype))
        for tag, two in (('mg', True), ('mg_levels', False)):
            mg = Multigrid(Ap2, coarsest=10, keep_host=True, two_launch=two)
            assert mg.nlevels >= 3, mg.sizes
            assert bool(mg.struct.C[0].rowptr) == two
            self.pre['p2', tag] = (mg, functools.partial(
                kr.vcycle, mg.host_levels, _host(mg._Ainv), mg.omega))
        for name in ('p2', 'block'):
            S = self.systems[name]
            pre = ilu.Ilu0(self.A[name])
            assert pre.packed is None
            n = S.n
            blocks = [S.A[k * n:(k + 1) * n, k * n:(k + 1) * n]
                      for k in range(S.N // n)]
            inv = kr.ilu0_inverse(blocks, pre.plan.host['old_of_new'])
            self.pre[name, 'ilu'] = (pre, functools.partial(kr.Dense, inv))
        self._measured = {}

    @staticmethod
    def _pattern(mesh, deg, with_stiffness):
        from flow_amd import fem
        from flow_amd.fem import ops
        V = fem.FunctionSpace(mesh, 'CG', deg)
        lay = V.layout
        rp = numpy.asarray(lay.pattern('rowptr'), dtype=numpy.int64)
        ci = numpy.asarray(lay.pattern('cols'), dtype=numpy.int64)
        out = [rp, ci, _host(ops.assemble_mass(V).vals)[:lay.nnz].copy()]
        if with_stiffness:
            out.append(_host(ops.assemble_stiffness(V).vals)[:lay.nnz].copy())
        return tuple(out), lay

    def map_of(self, case):
        S = self.systems[case['system']]
        if case['pre'] == 'none':
            return kr.identity
        if case['pre'] == 'jacobi':
            return lambda dtype: kr.jacobi(S.dinv, dtype)
        return self.pre[case['system'], case['pre']][1]

    def measured(self, case):
        '''On the host, reference against reference, with the conditions
        the systems were chosen for.'''
        if case['id'] not in self._measured:
            S, v = self.systems[case['system']], self.vecs[case['system']]
            m = kr.Measured(case, S, self.map_of(case), v)
            print('MEASURED %-40s N %6d K %2d d %.2e tol %.2e'
                  % (case['id'], S.N, m.K, m.d, m.tol))
            assert m.d * kr.MARGIN <= m.tol < 1.0e-7
            if case in kr.CASES:
                assert m.K >= kr.MIN_ITERATES
                restart = case['opts'].get('restart', 30)
                assert restart == 30 or m.K >= 2 * restart + 1
            b = v['b'].astype(kr.EXT)
            if case['start'] in ('kept', 'dropped'):
                r0 = b - S.op(kr.EXT)(v[case['start']].astype(kr.EXT))
                B = self.map_of(case)(kr.EXT)
                if case['start'] == 'kept':
                    assert kr.norm(r0) < 0.9 * kr.norm(b)
                    assert kr.norm(B(r0)) < 0.9 * kr.norm(B(b))
                else:
                    assert kr.norm(r0) > 10.0 * kr.norm(b)
            self._measured[case['id']] = m
        return self._measured[case['id']]

    def solve(self, hip, case, maxit, rtol=0.0, check_every=1, first_check=0,
              verify=None):
        '''One call of the C ABI from a fresh start and a workspace of NaN:
        (return code, iterations, residual, x on the host).'''
        import torch
        from flow_amd import _hip
        name, solver, opts = case['system'], case['solver'], case['opts']
        A, S = self.A[name], self.systems[name]
        N = S.N
        v = self.vecs[name]
        b = _dev(v[opts.get('b', 'b')])
        x = _dev(v[case['start']].copy())
        pre = self.pre.get((name, case['pre']), (None,))[0]
        dinv = None if case['pre'] in ('none', 'ilu') else \
            _hip.f64(self.dinv[name], N, 'dinv')
        op = A.operator()
        restart = opts.get('restart', 30)
        nparts = op.nblocks * (2 if A.kind == 1 else 1) + 2
        size = _hip.REDUCE_WORK + 64 + {
            'cg': 5 * N + nparts + (2 * pre.struct.lda if case['pre'] ==
                                    'two_level' else 0)
            + (2 * max(pre.struct.Ps[0].nblocks, pre.struct.up_nblocks[0])
               if case['pre'].startswith('mg') else 0),
            'bicgstab': 8 * N,
            'gmres': (2 * restart + 2) * N + _hip.GMRES_PARTIALS
            + _hip.GMRES_STATE}[solver]
        wk = torch.full((size,), float('nan'), dtype=torch.float64,
                        device=x.device)
        its, res = ctypes.c_int(-1), ctypes.c_double(-1.0)
        tail = (_hip.f64(wk), wk.numel(), ctypes.byref(its), ctypes.byref(res))
        if solver == 'cg':
            two = ctypes.byref(pre.struct) if case['pre'] == 'two_level' else None
            mg = ctypes.byref(pre.struct) if case['pre'].startswith('mg') else None
            head = (ctypes.byref(op), dinv, two, mg, _hip.f64(b, N), _hip.f64(x, N))
            ctl = (float(rtol), 0.0, int(maxit), int(check_every), int(first_check))
            if opts.get('guarded'):
                dropped = ctypes.c_int(-1)
                rc = hip.flow_cg_solve_guarded(
                    *(head + (None,) + ctl + tail
                      + (ctypes.byref(dropped), _hip.stream())))
                assert dropped.value == 0, 'a kept start was dropped'
            else:
                rc = hip.flow_cg_solve(*(head + ctl + tail + (_hip.stream(),)))
        elif solver == 'bicgstab':
            rc = hip.flow_bicgstab_solve(
                ctypes.byref(op), dinv,
                ctypes.byref(pre.struct) if case['pre'] == 'ilu' else None,
                _hip.f64(b, N), _hip.f64(x, N), float(rtol), 0.0, int(maxit),
                int(check_every), int(first_check), *(tail + (_hip.stream(),)))
        else:
            if verify is None:
                verify = opts.get('verify', 1)
            rc = hip.flow_gmres_solve(
                ctypes.byref(op), dinv,
                ctypes.byref(pre.struct) if case['pre'] == 'ilu' else None, None,
                _hip.f64(b, N), _hip.f64(x, N), float(rtol), 0.0, int(maxit),
                int(restart), int(opts.get('x_is_zero', 0)), int(first_check),
                int(verify), *(tail + (_hip.stream(),)))
        assert rc in (FLOW_OK, FLOW_NOT_CONVERGED), _hip.load_library(
            ).flow_last_error()
        return rc, its.value, res.value, _host(x)


@pytest.fixture(scope='module')
def W(hip):
    return World()


def _compare(tag, got, ref, k, tol):
    '''(its, res, x) of the device against iterate k of the reference.'''
    its, res, x = got
    assert its == k, '%s: reports %d iterations for maxit %d' % (tag, its, k)
    assert numpy.isfinite(x).all(), '%s iterate %d' % (tag, k)
    e2, emax = kr.rel(x, ref.xs[k]), kr.rel_max(x, ref.xs[k])
    er = kr.rel(res, ref.norms[k])
    print('ITERATE %s k %2d  l2 %.2e  max %.2e  norm %.2e  (tol %.2e)'
          % (tag, k, e2, emax, er, tol))
    assert e2 <= tol and emax <= tol, \
        '%s: x departs at iterate %d: %.3e l2, %.3e max > %.3e' % (
            tag, k, e2, emax, tol)
    assert er <= tol, '%s: the reported norm of iterate %d: %.17g, ' \
        'reference %.17g' % (tag, k, res, float(ref.norms[k]))


@pytest.mark.parametrize('case', kr.CASES, ids=lambda c: c['id'])
def test_every_iterate(hip, W, case):
    m = W.measured(case)          # (host only: before the device is asked)
    for k in range(m.K + 1):
        rc, its, res, x = W.solve(hip, case, maxit=k)
        assert rc == FLOW_NOT_CONVERGED, (case['id'], k, rc)
        _compare(case['id'], (its, res, x), m.ext, k, m.tol)
    # one batch planned past maxit: the same iterate, count and norm
    rc, its, res, x = W.solve(hip, case, maxit=m.K, first_check=m.K + 5,
                              check_every=m.K + 5)
    assert rc == FLOW_NOT_CONVERGED
    _compare(case['id'] + ' one batch', (its, res, x), m.ext, m.K, m.tol)


def test_the_dropped_start_runs_the_trajectory_from_zero(W):
    a = W.measured(kr.CASES[[c['id'] for c in kr.CASES].index(
        'gmres-block-jacobi-dropped-r4')])
    b = W.measured(kr.CASES[[c['id'] for c in kr.CASES].index(
        'gmres-block-jacobi-zero-r4')])
    assert kr.departure(a.ext, b.ext, min(a.K, b.K)) == 0.0


@pytest.mark.parametrize('case', kr.COUNT_CASES, ids=lambda c: c['id'])
def test_counts(hip, W, case):
    '''rtol between the reference's relative residuals at k* - 1 and k* (a
    factor >= 10 apart): every batching reports k*, leaves iterate k* and its
    norm.'''
    m = W.measured(case)
    kstar, rtol, rels = kr.count_target(m.ext, case['solver'])
    assert rels[kstar - 1] >= 10.0 * rels[kstar]
    assert min(rels[:kstar]) >= 3.0 * rtol >= 9.0 * rels[kstar]
    tol = kr.count_tolerance(m, kstar)
    assert tol < 1.0e-7
    gm = case['solver'] == 'gmres'
    if gm:
        true = float(m.ext.norms[kstar])
        assert abs(float(m.ext.est[kstar]) - true) <= 0.01 * true
    for verify in ((1, 0) if gm else (1,)):
        for check_every, first_check in ((1, 0), (50, 50)):
            rc, its, res, x = W.solve(hip, case, maxit=200, rtol=rtol,
                                      check_every=check_every,
                                      first_check=first_check, verify=verify)
            tag = '%s verify %d batch %d' % (case['id'], verify, first_check)
            assert rc == FLOW_OK, tag
            assert its == kstar, '%s: %d iterations, reference %d' % (
                tag, its, kstar)
            e2, emax = kr.rel(x, m.ext.xs[kstar]), kr.rel_max(x, m.ext.xs[kstar])
            er = kr.rel(res, m.ext.norms[kstar])
            print('COUNT %s l2 %.2e max %.2e norm %.2e (tol %.2e)'
                  % (tag, e2, emax, er, tol))
            assert e2 <= tol and emax <= tol, tag
            # (verify = 0 reports the least-squares estimate)
            assert er <= (tol if verify else 0.01), tag


@pytest.mark.parametrize('which', ['two_level', 'mg', 'mg_levels', 'ilu-p2',
                                   'ilu-block'])
def test_preconditioners_are_the_explicit_maps(hip, W, which):
    from flow_amd import _hip, device
    pre, _, name = which.partition('-')
    name = name or 'p2'
    S = W.systems[name]
    obj, B = W.pre[name, pre]
    r = numpy.random.RandomState(77).standard_normal(S.N)
    z = _dev(numpy.full(S.N, numpy.nan))
    rd = _dev(r)
    if pre == 'two_level':
        wk = _dev(numpy.full(2 * obj.struct.lda, numpy.nan))
        _hip.check(hip.flow_two_level_apply(
            ctypes.byref(obj.struct), _hip.f64(W.dinv[name], S.N),
            _hip.f64(rd, S.N), _hip.f64(z, S.N), _hip.f64(wk), _hip.stream()))
    elif pre == 'ilu':
        obj.solve(rd, z)
    else:
        obj.apply(rd, z)
    err = kr.rel(_host(z), B(kr.EXT)(r.astype(kr.EXT)))
    print('MAP %s %.3e' % (which, err))
    assert err <= 1.0e-12


def test_reductions_take_a_second_pass(hip):
    '''dot3_kernel above kRedBlocks blocks of 4 kBlock entries: n = 2^20 + 257.
    The entries carry 24-bit mantissas: every product is exact in fp64 and
    math.fsum of them is the correctly rounded sum.'''
    import math
    from flow_amd.fem import ops
    n = 1048576 + 257
    rng = numpy.random.RandomState(5)
    x = rng.standard_normal(n).astype(numpy.float32).astype(numpy.float64)
    y = rng.standard_normal(n).astype(numpy.float32).astype(numpy.float64)
    x[-3] = 16.0                  # (the maximum lies behind the first pass)
    xd, yd = _dev(x), _dev(y)
    eps = 2.0**-53
    want = math.fsum(x * y)
    assert abs(ops.dot(xd, yd) - want) <= n * eps * math.fsum(abs(x * y))
    sq = math.fsum(x * x)
    assert abs(ops.vector_norm(xd, 'l2') - math.sqrt(sq)) <= \
        n * eps * math.sqrt(sq)
    assert ops.vector_norm(xd, 'linf') == 16.0 == abs(x).max()
