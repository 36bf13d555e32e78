# -*- coding: utf-8 -*-
'''
The fp64 CSR-stream products row by row (-m gpu): StreamTile, stream_rows_sum
and stream_tile_pair_row_sum of flow_amd/csrc/csr_stream.h and the hand-inlined
copy in spmv_stream_block2_kernel, on synthetic patterns that put tiles at both
parities of their first nonzero, at the cap, around a group of xcd_tile, at an
odd end of the plane and -- for the rectangular operators -- on empty rows and
empty tiles (tests/fp64_stream_reference.py; what the comparisons can and
cannot see: tests/test_fp64_streams_host.py).

(1) flow_operator_apply, kinds 0, 1, 2, 4, and kind 0 on the rectangular
patterns; (2) flow_operator_apply_block_chunk; (3) the mass residuals
mass_residual_kernel / mass_residual_pair_kernel through one correction of
MassSolver.solve from a nonzero start (rho0 stays in plane 0 of work16: the
correction reads it and writes the other planes); (4) mg_level_kernel<0>,
mg_level_kernel<1>, mg_up2_kernel and the product with C through flow_mg_apply
on a hand-built two-level flow_mg.  The DOTS instances of the multigrid
kernels are only launched from inside flow_cg_solve and stay out of scope.

Exact data (small integers) is compared bit for bit with an integer model,
every row; random data with the bound (len + c) 2^-53 sum |v| |x| against the
correctly rounded row sums.  The device structs are the product's own
(ops.Matrix over a stub layout, multigrid.CsrOperator): padding and alignment
are the product's rules.
'''
import ctypes
import functools

import numpy
import pytest

import fp64_stream_reference as ref

pytestmark = pytest.mark.gpu

GUARD = 8                       # entries behind a result that must stay as set
SENTINEL = -7.25e11
BLOCK_PATTERNS = ('parity', 'full', 'odd_end', 'odd_end_n1', 'odd_end_n333')


def _dev(a):
    from flow_amd import device
    return device.to_device(numpy.ascontiguousarray(a))


def _host(t):
    from flow_amd import device
    return device.to_host(t).numpy()


@functools.lru_cache(maxsize=None)
def _layout(name, cap):
    return ref.StubLayout(ref.square(name, cap))


def _matrix(p, lay, kind, planes, mask=None, poison=True):
    '''ops.Matrix of `kind` over the pattern; poison: the one readable entry
    behind every value plane (plane_stride's padding, where nnz is odd) is NaN
    instead of 0.'''
    from flow_amd.fem import ops
    nplanes = ops.Matrix.NPLANES[kind]
    stride = ops.plane_stride(lay)
    host = numpy.zeros((nplanes, stride))
    host[:, :p.nnz] = planes[:nplanes]
    if poison:
        host[:, p.nnz:] = numpy.nan
    return ops.Matrix(lay, kind, _dev(host.reshape(-1)),
                      rowmask=_dev(mask) if kind == 4 else None)


def _guarded(size):
    return _dev(numpy.full(size + GUARD, SENTINEL))


def _result(y, size, what):
    out = _host(y)
    assert (out[size:] == SENTINEL).all(), what + ': written behind the result'
    return out[:size]


def _apply(A, x):
    y = _guarded(A.size)
    A.apply(_dev(numpy.asarray(x, dtype=numpy.float64)), y)
    return _result(y, A.size, 'apply')


def _apply_three_ways(p, lay, kind, planes, x, mask):
    '''apply with the padding behind the planes zero, NaN, and NaN again: the
    same bits, all finite.'''
    y0 = _apply(_matrix(p, lay, kind, planes, mask, poison=False), x)
    A = _matrix(p, lay, kind, planes, mask)
    y1, y2 = _apply(A, x), _apply(A, x)
    assert numpy.isfinite(y0).all()
    assert numpy.array_equal(ref.bits(y1), ref.bits(y0)), 'the padding is used'
    assert numpy.array_equal(ref.bits(y2), ref.bits(y1)), 'two calls differ'
    return y0


def _square_case(name, kind):
    cap = ref.tile_cap(kind)
    p = ref.square(name, cap)
    size = p.n * (1 if kind == 0 else 2)
    mask = ref.row_mask(p) if kind == 4 else None
    return p, _layout(name, cap), size, mask


# -- (1) flow_operator_apply ------------------------------------------------------------
@pytest.mark.parametrize('kind', [0, 1, 2, 4])
@pytest.mark.parametrize('name', ref.SQUARE)
def test_apply_exact_data_bit_for_bit(hip, name, kind):
    p, lay, size, mask = _square_case(name, kind)
    v, x = ref.exact_data(p, 100 + kind)
    x = x[:size]
    want, sabs = ref.int_product(kind, p, v, x, mask)
    ref.assert_exact(sabs, '%s kind %d' % (name, kind))
    got = _apply_three_ways(p, lay, kind, v, x, mask)
    ref.assert_bits(got, want, 'apply %s kind %d' % (name, kind))
    if kind == 4:
        ident = mask == 0
        assert ident.any() or p.n < 4
        assert numpy.array_equal(ref.bits(got[ident]),
                                 ref.bits(x[ident].astype(numpy.float64)))


@pytest.mark.parametrize('kind', [0, 1, 2, 4])
@pytest.mark.parametrize('name', ref.SQUARE)
def test_apply_random_data_row_by_row(hip, name, kind):
    p, lay, size, mask = _square_case(name, kind)
    v, x = ref.random_data(p, 200 + kind)
    x = x[:size]
    want, bound = ref.float_product(kind, p, v, x, mask)
    got = _apply_three_ways(p, lay, kind, v, x, mask)
    tag = 'fp64 apply kind %d %s' % (kind, name)
    worst = ref.assert_rows(got, want, bound, tag)
    print('RATIO %s %.3g' % (tag, worst))
    if kind == 4:
        assert numpy.array_equal(ref.bits(got[mask == 0]), ref.bits(x[mask == 0]))


def _csr_operator(p, vals, hand):
    '''multigrid.CsrOperator over a rectangular pattern; hand: the pattern's
    hand-picked tiles in place of the operator's own partition.'''
    from flow_amd import _hip
    from flow_amd.fem.multigrid import CsrOperator
    op = CsrOperator(p.scipy(numpy.asarray(vals, dtype=numpy.float64)))
    assert op.op.nnz == p.nnz and op.op.n == p.n
    own = _host(op._rb)
    ref.check_preconditions(p, own)
    if hand:
        assert not numpy.array_equal(own, p.rowblocks)
        op._hand = _dev(p.rowblocks)
        op.op.rowblocks = _hip.i32(op._hand)
        op.op.nblocks = len(p.rowblocks) - 1
    return op


@pytest.mark.parametrize('data', ['exact', 'random'])
@pytest.mark.parametrize('tiles', ['hand', 'own'])
@pytest.mark.parametrize('name', ref.RECT)
def test_apply_rectangular_with_empty_rows_and_tiles(hip, name, tiles, data):
    from flow_amd import _hip
    p = ref.rect(name, ref.tile_cap(0))
    make = ref.exact_data if data == 'exact' else ref.random_data
    v, x = make(p, 250, planes=1, ncomp=1)
    op = _csr_operator(p, v[0], tiles == 'hand')
    y = _guarded(p.n)
    xd = _dev(x.astype(numpy.float64))
    for _ in range(2):
        _hip.check(hip.flow_operator_apply(
            ctypes.byref(op.op), _hip.f64(xd, p.shape[1]), _hip.f64(y, p.n),
            _hip.stream()))
    got = _result(y, p.n, name)
    tag = 'fp64 apply rectangular %s %s' % (name, tiles)
    if data == 'exact':
        want, sabs = ref.int_product(0, p, v, x)
        ref.assert_exact(sabs, name)
        ref.assert_bits(got, want, tag)
    else:
        want, bound = ref.float_product(0, p, v, x)
        print('RATIO %s %.3g' % (tag, ref.assert_rows(got, want, bound, tag)))
    assert (got[p.lens == 0] == 0.0).all() and (p.lens == 0).sum() > 100


# -- (2) flow_operator_apply_block_chunk ----------------------------------------------------
@pytest.mark.parametrize('chunk', [0, 2, 4, 8])
@pytest.mark.parametrize('name', BLOCK_PATTERNS)
def test_apply_block_every_column_against_the_integer_model(hip, name, chunk):
    p, lay, n, _ = _square_case(name, 0)
    v, _x = ref.exact_data(p, 300)
    A = _matrix(p, lay, 0, v)
    rng = numpy.random.RandomState(301 + chunk)
    # (chunk 0: the library's choice, two columns at a time)
    for m in (1, (chunk or 2) + 1):
        ldx, ldy = n + (n & 1) + 2, n + (n & 1) + 4
        X = numpy.full((m, ldx), numpy.nan)          # (the padding: never read)
        xi = rng.randint(-ref.EXACT_MAG, ref.EXACT_MAG + 1, size=(m, n))
        xi[rng.uniform(size=xi.shape) < 0.1] = 0
        X[:, :n] = xi
        Y = _dev(numpy.full((m, ldy), SENTINEL).reshape(-1))
        A.apply_block(_dev(X.reshape(-1)), ldx, m, Y, ldy, chunk=chunk)
        got = _host(Y).reshape(m, ldy)
        assert (got[:, n:] == SENTINEL).all(), 'written behind a column'
        for j in range(m):
            want, sabs = ref.int_product(0, p, v, xi[j].astype(numpy.int64))
            ref.assert_exact(sabs, name)
            ref.assert_bits(got[j, :n], want, 'apply_block %s chunk %d m %d '
                            'column %d' % (name, chunk, m, j))
        assert numpy.array_equal(ref.bits(got[0, :n]),
                                 ref.bits(_apply(A, xi[0])))


# -- (3) the mass residuals -------------------------------------------------------------------
@pytest.mark.parametrize('kind', [0, 4], ids=['scalar', 'pair'])
@pytest.mark.parametrize('name', BLOCK_PATTERNS)
def test_mass_residuals_bit_for_bit(hip, name, kind):
    '''rho0 = float(dinv (b - A x)) of ONE correction from a nonzero integer
    start, dinv powers of two: plane 0 of work16.  (Not a mass matrix: the
    correction does not meet rtol = 0.)'''
    from flow_amd import _hip
    from flow_amd.fem import mass as fmass
    p, lay, size, mask = _square_case(name, kind)
    n, ncomp = p.n, size // p.n
    v, x = ref.exact_data(p, 400 + kind)
    x = x[:size]
    rng = numpy.random.RandomState(410 + kind)
    b = rng.randint(-ref.EXACT_MAG, ref.EXACT_MAG + 1, size=size).astype(numpy.int64)
    dinv = 2.0**-rng.randint(0, 5, size=size)
    Ax, sabs = ref.int_product(kind, p, v, x, mask)
    ref.assert_exact(sabs + numpy.abs(b), name + ' residual', grid=4)
    A = _matrix(p, lay, kind, v, mask)
    solver = fmass.MassSolver(A, _dev(dinv), steps=3)
    solver.guard = False
    xd = _dev(x.astype(numpy.float64))
    with pytest.raises(_hip.NotConverged):
        solver.solve(_dev(b.astype(numpy.float64)), xd, rtol=0.0, maxit=1)
    rho0 = _host(solver.work16)[:size].reshape(n, ncomp)
    want = numpy.float32(dinv * (b - Ax).astype(numpy.float64))
    ref.assert_bits(rho0, want.reshape(ncomp, n).T,
                    'mass residual %s kind %d' % (name, kind))
    if kind == 4 and n > 4:
        ident = (mask == 0).reshape(ncomp, n).T
        assert ident.any()
        own = numpy.float32(dinv * (b - x)).reshape(ncomp, n).T
        assert numpy.array_equal(ref.bits(rho0[ident]), ref.bits(own[ident]))


# -- (4) the multigrid level kernels ------------------------------------------------------------
def _cycle(hip, ops, fused, hand, identity):
    '''flow_mg_apply on a two-level flow_mg filled as Multigrid.__init__ fills
    it: dict of the device's t, r1, x1, z.'''
    from flow_amd import _hip
    from flow_amd.fem.multigrid import CsrOperator
    from flow_amd.fem.space import csr_stream_rowblocks
    n, nc = ref.MG_N, ref.MG_NC
    L = dict((k, _csr_operator(ops[k][0], ops[k][1], hand))
             for k in ('Ah', 'Ps', 'R'))
    M = _hip.MgS()
    M.nlevels = 2
    for field, key in ((M.Ah, 'Ah'), (M.Ps, 'Ps'), (M.R, 'R')):
        ctypes.memmove(ctypes.byref(field[0]), ctypes.byref(L[key].op),
                       ctypes.sizeof(_hip.Operator))
    keep = dict(dinv=_dev(2.0**-ops['dinv_exp'].astype(numpy.float64)),
                t=_dev(numpy.full(n, numpy.nan)),
                r1=_dev(numpy.full(nc, numpy.nan)),
                x1=_dev(numpy.full(nc, numpy.nan)))
    M.dinv[0] = _hip.f64(keep['dinv'], n).value
    M.t[0] = _hip.f64(keep['t'], n).value
    M.r[1] = _hip.f64(keep['r1'], nc).value
    M.x[1] = _hip.f64(keep['x1'], nc).value
    if fused:
        C = CsrOperator(ref.mg_restriction(ops))
        up = csr_stream_rowblocks([ops['Ps'][0].rowptr, ops['Ah'][0].rowptr])
        # (Ps keeps its empty tiles in the common partition)
        assert len(ref.empty_tiles(ops['Ps'][0], up)) >= 3
        keep.update(C=C, up=_dev(up))
        ctypes.memmove(ctypes.byref(M.C[0]), ctypes.byref(C.op),
                       ctypes.sizeof(_hip.Operator))
        M.up_rowblocks[0] = _hip.i32(keep['up']).value
        M.up_nblocks[0] = len(up) - 1
    lda = (nc + 3) // 4 * 4
    A32 = numpy.zeros((nc, lda), dtype=numpy.float32)
    if identity:
        A32[:, :nc] = numpy.eye(nc, dtype=numpy.float32)
    keep['Ainv'] = _dev(A32)
    M.nc, M.lda = nc, lda
    M.Ainv = _hip.f32(keep['Ainv'], nc * lda).value
    M.omega = 0.5
    z = _guarded(n)
    r = _dev(ops['r'].astype(numpy.float64))
    _hip.check(hip.flow_mg_apply(ctypes.byref(M), n, _hip.f64(r, n, 'r'),
                                 _hip.f64(z, n, 'z'), _hip.stream()))
    out = dict((k, _host(keep[k])) for k in ('t', 'r1', 'x1'))
    out['z'] = _result(z, n, 'mg')
    del L
    return out


@pytest.mark.parametrize('form', ['levels-hand', 'levels-own', 'two-launch'])
def test_multigrid_level_kernels_bit_for_bit(hip, form):
    '''non-fused: t = r - Ah r, r1 = R t, z = Ps r1 + w dinv (r + t)
    (mg_level_kernel<0>, the kind-0 product, mg_level_kernel<1>); two-launch:
    r1 = C r, z = Ps r1 + w dinv (2 r - Ah r) (the kind-0 product with C,
    mg_up2_kernel) -- with Ainv the fp32 identity, then 0 (the epilogue alone
    over Ps 0).'''
    ops = ref.mg_operators(ref.tile_cap(0))
    fused = form == 'two-launch'
    for identity in (True, False):
        m = ref.mg_model(ops, fused, identity)
        for stage, sabs in m['sabs'].items():
            ref.assert_exact(sabs, 'mg ' + stage)
        got = _cycle(hip, ops, fused, form == 'levels-hand', identity)
        tag = 'mg %s Ainv = %d ' % (form, identity)
        if fused:
            assert numpy.isnan(got['t']).all()        # (not written)
        else:
            ref.assert_bits(got['t'], m['t'], tag + 't')
        ref.assert_bits(got['r1'], m['r1'], tag + 'r1')
        ref.assert_bits(got['x1'], m['x1'], tag + 'x1')
        ref.assert_bits(got['z'], m['z32'].astype(numpy.float64) / 32.0, tag + 'z')
    assert m['r1'].any() and (m['z32'] % 32 != 0).any()
