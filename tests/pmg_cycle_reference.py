# -*- coding: utf-8 -*-
'''
An exact model of every launch of the p-multigrid / Chebyshev cycle
(`pmg_apply` in flow_amd/csrc/pmg_kernels.hip), the comparator that holds a
device -- or a stand-in for one -- against it, and the synthetic inputs
(helper, not a test; tests/test_pmg_cycle_host.py, tests/test_pmg_cycle_gpu.py).

The cycle leaves its work buffer behind.  Which launch is visible in it depends
on the step counts: with post = 1 the last launch writes only z, so the pre-
smoothing, the residual, the restriction's input and the prolongation's output
are all there; with coarse_steps = 1 the restriction's outputs are; coarse step
j takes its inputs from the run with coarse_steps = j and its outputs from the
run with j + 1 (what the two runs share is bitwise equal), and post-smoothing
step 2 of post = 3 takes its input rho from the run with post = 2.  `compare`
takes a dict of such runs and checks every launch it can see in them, every
row, with the bound of the fp16 stream products
    (len + 4) 2^-24 (sum |w| |g| + |epilogue operands|)
(tests/fp16_stream_reference.py) and, for the transfers, with (terms + 4) 2^-24
(sum |terms|).  Single fp32 operations are compared bit for bit.  MODE 2 has up
to seven epilogue roundings where the rule counts four: the rule is kept as
it is (a worst case no row attains; the fp32 stand-in stays below 0.5).

The model of a launch is float64 arithmetic on the vectors the device read,
widened exactly.  ONE intermediate cannot be read back: the in-place rho
between the pre-smoothing steps when pre >= 2 (`_pre_smoothing`).  There the
model chains the launches and ADDS the bound of the unobserved rho: rho enters
the next launch additively, never through a product, so the bounds add without
amplification.  Nowhere else.

`cycle_f32` is the same launches in fp32 without FMA, in row order, through
the work-buffer layout of pmg_apply -- the stand-in for a device in the host
tests, with the seeded defects (MUTATIONS) the comparator has to reject.
`cycle_f64` is the pure float64 composition with a composed first-order bound
(every launch's own bound plus the bounds of its inputs carried through its
linear map).
'''
from types import SimpleNamespace

import numpy

from fp16_stream_reference import (U32, assert_rows, blocked, cheb_coefficients,
                                   pmg_one_plane, pmg_two_planes, row_bound,
                                   tile_product, tile_product_f32)

K_AHEAD = 8                     # kAhead of pmg_restrict_kernel
SENTINEL = -7.25                # what z holds before the call
RATIO_FINE, RATIO_COARSE, SAFETY = 5.0, 12.0, 1.1   # the defaults of Pmg

# the minimum grid of (pre, post, coarse_steps) and what each group is for
GRID = (
    # init, pre-smoothing, MODE 0 x diag, restrict, prolong with 1 / 2 / 3
    # terms, MODE 2 with d_own and d_extra absent
    (1, 1, 1), (2, 1, 1), (3, 1, 1),
    # coarse steps 1, 2, 3 and 6: both parities of the ping-pong
    (1, 1, 2), (1, 1, 3), (1, 1, 4), (1, 1, 6), (1, 1, 7),
    # post-smoothing: MODE 1 without d_own, MODE 2 with d_own, with d_extra
    (1, 2, 1), (1, 3, 1),
    # everything at once: d[2] live, d[0] reused as d_extra
    (3, 1, 2), (3, 2, 2), (3, 3, 2),
    # the default and the optimum of tools/precond_lab.py
    (1, 2, 6), (2, 2, 4))


def family(pre, post, cs):
    '''The runs that expose every launch of (pre, post, cs): post = 1 with
    1 .. cs coarse steps, then post = 2 .. post.'''
    return tuple([(pre, 1, j) for j in range(1, cs + 1)]
                 + [(pre, p, cs) for p in range(2, post + 1)])


KINDS = ('init', 'pre', 'mode0', 'restrict', 'coarse', 'prolong', 'post',
         'z', 'chain', 'shared')

MUTATIONS = (
    'no_d_extra',               # d_extra dropped in post = 3
    'no_dc',                    # dc dropped from the prolongation at pre = 3
    'own_half',                 # own-dof weight 0.5 in the restriction
    'no_tail',                  # restriction entries beyond the 8th dropped
    'bcc_kept',                 # coarse Dirichlet rows not zeroed
    'c_swapped',                # c1 / c2 swapped
    'post_continues',           # post-smoothing continues the pre-smoothing's
                                # coefficient sequence
    'pingpong',                 # the coarse step reads cd[j & 1]
    'mode0_no_diag',            # MODE 0 not multiplied by diag
    'z_bc_x',                   # Dirichlet rows of z return x
    'bc_stride',                # the second component's bc at a wrong stride
    'scalar_z_tail',            # scalar mode writes z[n + r]
    'dummy_nonzero',            # the dummy coarse row is not zero
    'weight_ulp',               # one weight of one row off by one fp16 ulp
)


def _wide(a):
    return numpy.asarray(a).astype(numpy.float64)


def _f32(a):
    return numpy.asarray(a).astype(numpy.float32)


# -- the work buffer --------------------------------------------------------------
def work_size(n, n1):
    return 12 * n + 8 * n1 + 2


def split(work, n, n1):
    '''The vectors of pmg_apply inside its work buffer, as (rows, 2) views:
    rho0, rho, d0, d1, d2, x | crho, cd0, cd1, cx | dummy (the zero coarse row
    behind cx); `xc` = cx with the dummy row, as the prolongation indexes it.'''
    work = numpy.asarray(work)
    assert work.shape == (work_size(n, n1),)
    out = {}
    for i, name in enumerate(('rho0', 'rho', 'd0', 'd1', 'd2', 'x')):
        out[name] = work[2 * n * i:2 * n * (i + 1)].reshape(n, 2)
    c = 12 * n
    for i, name in enumerate(('crho', 'cd0', 'cd1', 'cx')):
        out[name] = work[c + 2 * n1 * i:c + 2 * n1 * (i + 1)].reshape(n1, 2)
    out['dummy'] = work[c + 8 * n1:].reshape(1, 2)
    out['xc'] = work[c + 6 * n1:].reshape(n1 + 1, 2)
    return out


def observe(work, z, n, n1, scalar):
    '''One run as the comparator takes it: copies of the work vectors, z as
    (n, 2) -- in scalar mode (n, 1) and `z_tail`, the second half of the
    2n-buffer the call was given.'''
    run = dict((k, v.copy()) for k, v in split(work, n, n1).items())
    z = numpy.asarray(z, dtype=numpy.float64)
    assert z.shape == (2 * n,)
    if scalar:
        run['z'], run['z_tail'] = z[:n].reshape(n, 1).copy(), z[n:].copy()
    else:
        run['z'] = blocked(z, n).copy()
    return run


# -- one launch each: [(name, expected, bound)]; bound None = bit for bit -----------
def init(dinv, r2, inv_theta, rho0_dev=None):
    '''pmg_init_kernel: rho0 = rho = float(r) * dinv, d0 = inv_theta * rho0 (of
    the device's own rho0 when given): single fp32 operations.'''
    rho0 = _f32(r2) * _f32(dinv)
    d0 = numpy.float32(inv_theta) * (rho0 if rho0_dev is None else
                                     _f32(rho0_dev))
    return [('rho0', rho0, None), ('rho', rho0, None), ('d0', d0, None)]


def cheb_step(L, mode, g, rho_in, c1=0.0, c2=0.0, d_own=None, x=None,
              d_extra=None, diag=None, rho_dev=None, d_dev=None, bc=None,
              r=None, rho_in_bound=0.0):
    '''pmg_cheb_kernel on level L, rho' = rho_in - A~ g:
    MODE 0  rho' (times diag when given)
    MODE 1  rho' ; d' = c1 d_own + c2 rho' ; x' = x + d' -- around the rho / d
            the device wrote (rho_dev, d_dev) where they can be read back, so
            that each line is one expression with its own bound
    MODE 2  z = x + d_own + d_extra + c1 d_own + c2 rho'; Dirichlet rows (bc)
            return r bit for bit (bound 0).
    rho_in_bound: the bound of an unobserved rho_in, added (see above).'''
    g, rho_in = _wide(g), _wide(rho_in)
    s, sabs = tile_product(L.rp, L.cols, L.w, g, idrows=L.idrows)
    lens = L.lens
    rho = rho_in - s
    res_abs = numpy.abs(rho_in) + sabs
    if mode == 0:
        if diag is None:
            return [('rho', rho, row_bound(lens, res_abs) + rho_in_bound)]
        dg = numpy.abs(_wide(diag))
        return [('rho', rho * _wide(diag),
                 row_bound(lens, res_abs * dg) + rho_in_bound * dg)]
    c1, c2 = float(c1), float(c2)
    own = numpy.zeros_like(rho) if d_own is None else _wide(d_own)
    if mode == 1:
        lines = [('rho', rho, row_bound(lens, res_abs) + rho_in_bound)]
        if rho_dev is not None:
            rd = _wide(rho_dev)
            lines.append(('d', c1 * own + c2 * rd,
                          row_bound(lens, numpy.abs(c1 * own)
                                    + numpy.abs(c2 * rd))))
        else:
            lines.append(('d', c1 * own + c2 * rho,
                          row_bound(lens, numpy.abs(c1 * own)
                                    + abs(c2) * res_abs)
                          + abs(c2) * rho_in_bound))
        if x is not None:
            xs, dd = _wide(x), _wide(d_dev)
            lines.append(('x', xs + dd,
                          row_bound(lens, numpy.abs(xs) + numpy.abs(dd))))
        return lines
    xs = _wide(x)
    ex = numpy.zeros_like(rho) if d_extra is None else _wide(d_extra)
    z = xs + own + ex + c1 * own + c2 * rho
    bz = row_bound(lens, numpy.abs(xs) + numpy.abs(own) + numpy.abs(ex)
                   + numpy.abs(c1 * own) + abs(c2) * res_abs) \
        + abs(c2) * rho_in_bound
    if bc is not None:
        z = numpy.where(bc != 0, _wide(r), z)
        bz = numpy.where(bc != 0, 0.0, bz)
    return [('z', z, bz)]


def _lists(rptr, rsrc):
    rptr = numpy.asarray(rptr, dtype=numpy.int64)
    L = numpy.diff(rptr)
    owner = numpy.repeat(numpy.arange(len(L)), L)
    first = numpy.zeros(len(rsrc), dtype=bool)
    first[rptr[:-1]] = True
    return rptr, L, owner, first


def restrict(rptr, rsrc, res, dinv_c, bcc, inv_theta_c, crho_dev=None):
    '''pmg_restrict_kernel: s = (res[own] + 0.5 sum res[edge dofs]) dinv_c, 0
    on the coarse Dirichlet rows; dc = xc = inv_theta_c * rhoc of the device's
    own rhoc, bit for bit.'''
    rptr, L, owner, first = _lists(rptr, rsrc)
    res, dinv_c = _wide(res), _wide(dinv_c)
    t = res[numpy.asarray(rsrc, dtype=numpy.int64)]
    own = t[first]
    e = numpy.zeros_like(own)
    eabs = numpy.zeros_like(own)
    numpy.add.at(e, owner[~first], t[~first])
    numpy.add.at(eabs, owner[~first], numpy.abs(t[~first]))
    s = (own + 0.5 * e) * dinv_c
    bound = (L[:, None] + 4.0) * U32 * (numpy.abs(own) + 0.5 * eabs) \
        * numpy.abs(dinv_c)
    s = numpy.where(bcc != 0, 0.0, s)
    bound = numpy.where(bcc != 0, 0.0, bound)
    dc = numpy.float32(inv_theta_c) * _f32(s if crho_dev is None else crho_dev)
    return [('crho', s, bound), ('cd0', dc, None), ('cx', dc, None)]


def prolong(ends, ds, xc):
    '''pmg_prolong_kernel: x = da (+ db) (+ dc) + 0.5 (xc[e0] + xc[e1]); xc has
    the dummy row behind it (block mode: it must read 0).'''
    e = numpy.asarray(ends, dtype=numpy.int64)
    xc = _wide(xc)
    terms = [_wide(d) for d in ds] + [0.5 * xc[e[:, 0]], 0.5 * xc[e[:, 1]]]
    x = sum(terms)
    bound = (len(terms) + 4.0) * U32 * sum(numpy.abs(t) for t in terms)
    return [('x', x, bound)]


# -- the same launches in fp32, without FMA, in row order ---------------------------
def init_f32(dinv, r2, inv_theta):
    rho0 = _f32(r2) * _f32(dinv)
    return dict(rho0=rho0, rho=rho0.copy(), d0=numpy.float32(inv_theta) * rho0)


def cheb_step_f32(L, mode, g, rho_in, c1=0.0, c2=0.0, d_own=None, x=None,
                  d_extra=None, diag=None, bc=None, r=None, mut=()):
    g, rho_in = _f32(g), _f32(rho_in)
    c1, c2 = numpy.float32(c1), numpy.float32(c2)
    s = tile_product_f32(L.rp, L.cols, L.w_f32(mut), g, idrows=L.idrows)
    rho = rho_in - s
    if mode == 0:
        if diag is not None and 'mode0_no_diag' not in mut:
            rho = rho * _f32(diag)
        return dict(rho=rho)
    d = c2 * rho
    own = numpy.zeros_like(rho)
    if d_own is not None:
        own = _f32(d_own)
        d = d + c1 * own
    if mode == 1:
        out = dict(rho=rho, d=d)
        if x is not None:
            out['x'] = _f32(x) + d
        return out
    extra = numpy.zeros_like(rho) if d_extra is None else _f32(d_extra)
    acc = _f32(x) + ((own + d) + extra)
    z = acc.astype(numpy.float64)
    if bc is not None:
        z = numpy.where(bc != 0, _f32(x).astype(numpy.float64)
                        if 'z_bc_x' in mut else _wide(r), z)
    return dict(z=z)


def restrict_f32(rptr, rsrc, res, dinv_c, bcc, inv_theta_c, mut=()):
    rptr, L, _owner, _first = _lists(rptr, rsrc)
    res = _f32(res)
    rsrc = numpy.asarray(rsrc, dtype=numpy.int64)
    s = res[rsrc[rptr[:-1]]]
    e = numpy.zeros_like(s)
    top = min(int(L.max()), K_AHEAD) if 'no_tail' in mut else int(L.max())
    for k in range(1, top):
        rows = numpy.nonzero(L > k)[0]
        e[rows] = e[rows] + res[rsrc[rptr[rows] + k]]
    if 'own_half' in mut:
        s = numpy.float32(0.5) * s
    s = (s + numpy.float32(0.5) * e) * _f32(dinv_c)
    if 'bcc_kept' not in mut:
        s = numpy.where(bcc != 0, numpy.float32(0.0), s)
    d0 = numpy.float32(inv_theta_c) * s
    return dict(crho=s, cd0=d0, cx=d0.copy())


def prolong_f32(ends, ds, xc):
    e = numpy.asarray(ends, dtype=numpy.int64)
    xc = _f32(xc)
    v = _f32(ds[0])
    for d in ds[1:]:
        v = v + _f32(d)
    return dict(x=v + numpy.float32(0.5) * (xc[e[:, 0]] + xc[e[:, 1]]))


# -- the cycle ----------------------------------------------------------------------
def _coefficients(L, count, exact=False):
    '''first() and `count` times next() of Cheb; exact: unrounded doubles.'''
    if not exact:
        return cheb_coefficients(L.lo, L.hi, count)
    theta, delta = 0.5 * (L.hi + L.lo), 0.5 * (L.hi - L.lo)
    sigma = theta / delta
    rho, steps = 1.0 / sigma, []
    for _ in range(count):
        rn = 1.0 / (2.0 * sigma - rho)
        steps.append((rn * rho, 2.0 * rn / delta))
        rho = rn
    return 1.0 / theta, steps


def _input_pairs(prob, r):
    '''(n, 2): what the lanes of pmg_init_kernel read of r (scalar mode: the
    one component in both lanes, whatever lies behind it).'''
    r = numpy.asarray(r, dtype=numpy.float64)
    n = prob.n
    if prob.scalar:
        return numpy.stack([r[:n], r[:n]], axis=1)
    return blocked(r[:2 * n], n)


def cycle_f32(config, prob, r, z, work=None, mut=()):
    '''pmg_apply with the fp32 twins: the launch sequence, the aliasing and the
    overwrites of the work buffer as in the product.  r: the fp64 input (2n;
    scalar mode reads its first n), z: a 2n buffer that is written in place.
    Returns the work buffer.'''
    pre, post, cs = config
    mut = frozenset(mut)
    F, C = prob.fine, prob.coarse
    n, n1 = prob.n, prob.n1
    if work is None:
        work = numpy.zeros(work_size(n, n1), dtype=numpy.float32)
    if 'dummy_nonzero' in mut:
        work[-2:] = 1.0
    w = split(work, n, n1)
    d = [w['d0'], w['d1'], w['d2']]
    cd = [w['cd0'], w['cd1']]
    r2 = _input_pairs(prob, r)
    c0, steps = _coefficients(F, 6)

    def coeff(seq, j):
        c1, c2 = seq[j]
        return (c2, c1) if 'c_swapped' in mut else (c1, c2)
    out = init_f32(F.dinv, r2, c0)
    w['rho0'][:], w['rho'][:], d[0][:] = out['rho0'], out['rho'], out['d0']
    for j in range(1, pre):
        c1, c2 = coeff(steps, j - 1)
        out = cheb_step_f32(F, 1, d[j - 1], w['rho'], c1, c2, d_own=d[j - 1],
                            mut=mut)
        w['rho'][:], d[j][:] = out['rho'], out['d']
    w['rho'][:] = cheb_step_f32(F, 0, d[pre - 1], w['rho'], diag=F.diag,
                                mut=mut)['rho']
    c0c, csteps = _coefficients(C, max(cs - 1, 1))
    out = restrict_f32(prob.rptr, prob.rsrc, w['rho'], C.dinv, prob.bcc, c0c,
                       mut=mut)
    w['crho'][:], cd[0][:], w['cx'][:] = out['crho'], out['cd0'], out['cx']
    for j in range(1, cs):
        c1, c2 = coeff(csteps, j - 1)
        dn = cd[j & 1]
        dc = cd[j & 1] if 'pingpong' in mut else cd[(j - 1) & 1]
        out = cheb_step_f32(C, 1, dc, w['crho'], c1, c2, d_own=dc, x=w['cx'],
                            mut=())
        w['crho'][:], dn[:], w['cx'][:] = out['rho'], out['d'], out['x']
    ds = d[:pre]
    if 'no_dc' in mut and pre > 2:
        ds = ds[:2]
    w['x'][:] = prolong_f32(prob.ends, ds, w['xc'])['x']
    # post-smoothing
    seq = steps[pre - 1:] if 'post_continues' in mut else steps
    bc = prob.bc
    if 'bc_stride' in mut:
        flat = numpy.concatenate([bc[:, 0], bc[:, 1]])
        bc = numpy.stack([bc[:, 0], flat[(n1 + numpy.arange(n)) % (2 * n)]],
                         axis=1)
    last = dict(bc=bc, r=r2, mut=mut)
    if post == 1:
        zz = cheb_step_f32(F, 2, w['x'], w['rho0'], 0.0, c0, x=w['x'],
                           **last)['z']
    else:
        out = cheb_step_f32(F, 1, w['x'], w['rho0'], 0.0, c0, mut=mut)
        w['rho'][:], d[0][:] = out['rho'], out['d']
        for j in range(1, post):
            c1, c2 = coeff(seq, j - 1)
            if j + 1 == post:
                extra = d[0] if j == 2 and 'no_d_extra' not in mut else None
                zz = cheb_step_f32(F, 2, d[j - 1], w['rho'], c1, c2,
                                   d_own=d[j - 1], x=w['x'], d_extra=extra,
                                   **last)['z']
            else:
                out = cheb_step_f32(F, 1, d[j - 1], w['rho'], c1, c2,
                                    d_own=d[j - 1], mut=mut)
                w['rho'][:], d[j][:] = out['rho'], out['d']
    z[:n] = zz[:, 0]
    if not prob.scalar or 'scalar_z_tail' in mut:
        z[n:2 * n] = zz[:, 1]
    return work


def cycle_f64(config, prob, r, exact=False):
    '''The cycle as the composition of the launch models in float64: (z, bound)
    as (n, 2).  The bound is composed to first order: every launch adds its own
    bound to the bounds of its inputs carried through its linear map (through
    |w| for a product).  exact: no fp32 anywhere -- dinv = 1 / diag, unrounded
    Chebyshev coefficients, r as given: the algorithm itself, for the
    comparison with the textbook cycle (the bound is meaningless then).'''
    pre, post, cs = config
    F, C = prob.fine, prob.coarse
    r2 = _input_pairs(prob, r)
    c0, steps = _coefficients(F, 3, exact)
    c0c, csteps = _coefficients(C, max(cs - 1, 1), exact)
    diag = _wide(F.diag)
    if exact:
        dinv, cdinv = 1.0 / diag, 1.0 / _wide(C.diag)
        rho0 = r2 * dinv
        d0 = c0 * rho0
    else:
        dinv, cdinv = _wide(F.dinv), _wide(C.dinv)
        out = init_f32(F.dinv, r2, c0)
        rho0, d0 = _wide(out['rho0']), _wide(out['d0'])
    zero = numpy.zeros_like(rho0)

    def product(L, g, bg):
        s, sabs = tile_product(L.rp, L.cols, L.w, g, idrows=L.idrows)
        return s, sabs, tile_product(L.rp, L.cols, L.w, bg, idrows=L.idrows)[1]

    def step(L, g, bg, rho, brho, own, bown, c1, c2):
        '''MODE 1: (rho', its bound, d', its bound).'''
        s, sabs, bs = product(L, g, bg)
        res_abs = numpy.abs(rho) + sabs
        rn = rho - s
        brn = row_bound(L.lens, res_abs) + brho + bs
        dn = c1 * own + c2 * rn
        bdn = row_bound(L.lens, numpy.abs(c1 * own) + abs(c2) * res_abs) \
            + abs(c1) * bown + abs(c2) * (brho + bs)
        return rn, brn, dn, bdn

    def last(g, bg, rho, brho, own, bown, c1, c2, x, bx, ex, bex):
        '''MODE 2.'''
        s, sabs, bs = product(F, g, bg)
        res_abs = numpy.abs(rho) + sabs
        z = x + own + ex + c1 * own + c2 * (rho - s)
        bz = row_bound(F.lens, numpy.abs(x) + numpy.abs(own) + numpy.abs(ex)
                       + numpy.abs(c1 * own) + abs(c2) * res_abs) \
            + bx + (1.0 + abs(c1)) * bown + bex + abs(c2) * (brho + bs)
        return (numpy.where(prob.bc != 0, r2, z),
                numpy.where(prob.bc != 0, 0.0, bz))
    # pre-smoothing, residual times the diagonal
    d, bd = [d0], [zero]
    rho, brho = rho0, zero
    for j in range(1, pre):
        c1, c2 = steps[j - 1]
        rho, brho, dn, bdn = step(F, d[-1], bd[-1], rho, brho, d[-1], bd[-1],
                                  float(c1), float(c2))
        d.append(dn)
        bd.append(bdn)
    s, sabs, bs = product(F, d[-1], bd[-1])
    res = (rho - s) * diag
    bres = (row_bound(F.lens, numpy.abs(rho) + sabs) + brho + bs) \
        * numpy.abs(diag)
    # restriction (its bound with the list lengths; the scaling with
    # inv_theta_c is one more rounding)
    rptr, L, owner, first = _lists(prob.rptr, prob.rsrc)
    crho, bcr = restrict(prob.rptr, prob.rsrc, res, cdinv, prob.bcc, c0c)[0][1:]
    tb = bres[numpy.asarray(prob.rsrc, dtype=numpy.int64)]
    carried = tb[first].copy()
    half = numpy.zeros_like(carried)
    numpy.add.at(half, owner[~first], tb[~first])
    bcr = bcr + numpy.where(prob.bcc != 0, 0.0,
                            (carried + 0.5 * half) * numpy.abs(cdinv))
    dc = float(c0c) * crho
    bdc = U32 * numpy.abs(dc) + abs(float(c0c)) * bcr
    xc, bxc = dc, bdc
    for j in range(1, cs):
        c1, c2 = csteps[j - 1]
        crho, bcr, dn, bdn = step(C, dc, bdc, crho, bcr, dc, bdc, float(c1),
                                  float(c2))
        bxc = row_bound(C.lens, numpy.abs(xc) + numpy.abs(dn)) + bxc + bdn
        xc = xc + dn
        dc, bdc = dn, bdn
    # prolongation (the dummy row: an exact zero)
    pad = numpy.zeros((1, 2))
    xc, bxc = numpy.concatenate([xc, pad]), numpy.concatenate([bxc, pad])
    e = numpy.asarray(prob.ends, dtype=numpy.int64)
    (_, x, bx), = prolong(prob.ends, d, xc)
    bx = bx + sum(bd) + 0.5 * (bxc[e[:, 0]] + bxc[e[:, 1]])
    # post-smoothing
    if post == 1:
        return last(x, bx, rho0, zero, zero, zero, 0.0, float(c0), x, bx,
                    zero, zero)
    rho, brho, d0, bd0 = step(F, x, bx, rho0, zero, zero, zero, 0.0, float(c0))
    if post == 2:
        c1, c2 = steps[0]
        return last(d0, bd0, rho, brho, d0, bd0, float(c1), float(c2), x, bx,
                    zero, zero)
    c1, c2 = steps[0]
    rho, brho, d1, bd1 = step(F, d0, bd0, rho, brho, d0, bd0, float(c1),
                              float(c2))
    c1, c2 = steps[1]
    return last(d1, bd1, rho, brho, d1, bd1, float(c1), float(c2), x, bx, d0,
                bd0)


# -- the comparator -----------------------------------------------------------------
class Checker(object):
    '''assert_rows per line, the worst error / bound per launch kind.'''

    def __init__(self, tag):
        self.tag = tag
        self.worst = {}

    def rows(self, kind, got, want, bound, what):
        what = '%s %s %s' % (self.tag, kind, what)
        if bound is None:
            # bit for bit: a zero bound asks for equality; the signs of zeros
            # and the width of the type on top
            got, want = numpy.asarray(got), numpy.asarray(want)
            assert got.dtype == want.dtype and got.shape == want.shape, what
            ratio = assert_rows(got, want, 0.0, what)
            assert numpy.array_equal(numpy.signbit(got), numpy.signbit(want)), \
                what + ': differs bit for bit (sign of a zero)'
        else:
            want = numpy.asarray(want)
            ratio = assert_rows(numpy.asarray(got).reshape(want.shape), want,
                                bound, what)
        self.worst[kind] = max(ratio, self.worst.get(kind, 0.0))

    def lines(self, kind, got, lines, what, only=None):
        for name, want, bound in lines:
            if name in got and (only is None or name in only):
                self.rows(kind, got[name], want, bound, '%s %s' % (what, name))

    def report(self):
        for kind in KINDS:
            if kind in self.worst:
                print('RATIO %s %s %.3g' % (self.tag, kind, self.worst[kind]))
        return dict(self.worst)


def _pre_smoothing(ck, prob, run, pre, what):
    '''Pre-smoothing steps 1 .. pre - 1 and the residual (MODE 0 x diag) of a
    run with post = 1.  THE place where the model chains launches: the rho a
    step leaves in place is overwritten by the next one, so from the second
    product on rho_in is the model's own and its bound is added to the bounds
    of what is formed from it.  It enters additively: no amplification.'''
    F = prob.fine
    _c0, steps = _coefficients(F, 3)
    d = [run['d0'], run['d1'], run['d2']]
    rho, brho = _wide(run['rho0']), 0.0        # (init: rho = rho0, same lanes)
    for j in range(1, pre):
        c1, c2 = steps[j - 1]
        lines = cheb_step(F, 1, d[j - 1], rho, c1, c2, d_own=d[j - 1],
                          rho_in_bound=brho)
        ck.lines('pre', {'d': d[j]}, lines, '%s step %d' % (what, j))
        (_, rho, brho), = [ln for ln in lines if ln[0] == 'rho']
    ck.lines('mode0', {'rho': run['rho']},
             cheb_step(F, 0, d[pre - 1], rho, diag=F.diag, rho_in_bound=brho),
             what)


def _same(ck, a, b, names, what):
    for name in names:
        ck.rows('shared', a[name], b[name], None, '%s %s' % (what, name))


def compare(prob, r, runs, tag):
    '''Every launch that the runs {(pre, post, coarse_steps): run} expose,
    every row; returns the worst error / bound per launch kind.'''
    ck = Checker(tag)
    F, C = prob.fine, prob.coarse
    n = prob.n
    r2 = _input_pairs(prob, r)
    c0, steps = _coefficients(F, 3)
    for cfg in sorted(runs):
        pre, post, cs = cfg
        run = runs[cfg]
        # what this run writes (the rest of the buffer is left over from
        # earlier calls): d[j] of the pre-smoothing, d[1] of post = 3, cd[1]
        # from the second coarse step on
        pre_d = ('d0', 'd1', 'd2')[:pre]
        fine_names = ('rho0', 'rho') + pre_d + (
            ('d1',) if post == 3 and pre == 1 else ())
        coarse_names = ('crho', 'cd0', 'cx') + (('cd1',) if cs > 1 else ())
        what = '%d/%d/%d' % cfg
        d = [run['d0'], run['d1'], run['d2']]
        c0c, csteps = _coefficients(C, max(cs - 1, 1))
        # what every run shows
        for name in fine_names + coarse_names + ('x', 'z'):
            assert numpy.isfinite(run[name]).all(), (what, name)
        if prob.scalar:
            for name in fine_names + coarse_names + ('x',):
                ck.rows('shared', run[name][:, 1], run[name][:, 0], None,
                        what + ' lane y == lane x of ' + name)
            ck.rows('z', run['z_tail'], numpy.full(n, SENTINEL), None,
                    what + ' behind z (scalar mode: n entries)')
        lanes = slice(0, 1) if prob.scalar else slice(0, 2)
        zgot = {'z': run['z']}

        def zlines(lines):
            return [(nm, want[:, lanes], bound[:, lanes])
                    for nm, want, bound in lines]
        ck.lines('init', run, init(F.dinv, r2, c0, run['rho0']), what,
                 only=('rho0',) if post > 1 else ('rho0', 'd0'))
        if post == 1:
            _pre_smoothing(ck, prob, run, pre, what)
            if cs == 1:
                ck.lines('restrict', run, restrict(
                    prob.rptr, prob.rsrc, run['rho'], C.dinv, prob.bcc, c0c,
                    run['crho']), what)
            # (the dummy row behind cx reads 0 in the model, whatever the
            # device holds there)
            ck.lines('prolong', run, prolong(
                prob.ends, d[:pre],
                numpy.concatenate([run['cx'], numpy.zeros((1, 2))])), what)
            ck.lines('z', zgot, zlines(cheb_step(
                F, 2, run['x'], run['rho0'], 0.0, c0, x=run['x'], bc=prob.bc,
                r=r2)), what)
        if post >= 2 and (pre, 1, cs) in runs:
            _same(ck, runs[(pre, 1, cs)], run,
                  ('rho0', 'x') + coarse_names + pre_d[2:]
                  + (pre_d[1:2] if post == 2 else ()), what + ' as post = 1:')
        if post == 2:
            # first launch: MODE 1 without d_own, rho_out = rho, d_out = d[0]
            ck.lines('post', {'rho': run['rho'], 'd': d[0]}, cheb_step(
                F, 1, run['x'], run['rho0'], 0.0, c0, rho_dev=run['rho']),
                what + ' step 1')
            c1, c2 = steps[0]
            ck.lines('z', zgot, zlines(cheb_step(
                F, 2, d[0], run['rho'], c1, c2, d_own=d[0], x=run['x'],
                bc=prob.bc, r=r2)), what)
        if post == 3:
            # step 2 reads the rho that step 1 wrote: the one the run with
            # post = 2 still holds; d[0] and x are the same in both
            assert (pre, 2, cs) in runs, 'post = 3 needs the run with post = 2'
            two = runs[(pre, 2, cs)]
            _same(ck, two, run, ('rho0', 'd0', 'x') + coarse_names + pre_d[2:],
                  what + ' as post = 2:')
            c1, c2 = steps[0]
            ck.lines('post', {'rho': run['rho'], 'd': d[1]}, cheb_step(
                F, 1, d[0], two['rho'], c1, c2, d_own=d[0],
                rho_dev=run['rho']), what + ' step 2')
            c1, c2 = steps[1]
            ck.lines('z', zgot, zlines(cheb_step(
                F, 2, d[1], run['rho'], c1, c2, d_own=d[1], x=run['x'],
                d_extra=d[0], bc=prob.bc, r=r2)), what)
        # coarse step j = cs: inputs of this run, outputs of the run with one
        # step more
        nxt = runs.get((pre, post, cs + 1))
        if post == 1 and nxt is not None:
            j = cs
            old, new = 'cd%d' % ((j - 1) & 1), 'cd%d' % (j & 1)
            _same(ck, run, nxt, ('rho0', 'rho') + pre_d + (old,),
                  what + ' as %d coarse steps:' % (cs + 1))
            c1, c2 = _coefficients(C, j)[1][j - 1]
            ck.lines('coarse', {'rho': nxt['crho'], 'd': nxt[new],
                                'x': nxt['cx']},
                     cheb_step(C, 1, run[old], run['crho'], c1, c2,
                               d_own=run[old], x=run['cx'],
                               rho_dev=nxt['crho'], d_dev=nxt[new]),
                     what + ' coarse step %d' % j)
        # the dummy coarse row is still zero
        ck.rows('prolong', run['dummy'], numpy.zeros((1, 2), numpy.float32),
                None, what + ' dummy coarse row')
        # the whole cycle against the chained model
        zc, bzc = cycle_f64(cfg, prob, r)
        ck.rows('chain', run['z'], zc[:, lanes], bzc[:, lanes], what + ' z')
    return ck.report()


# -- inputs -------------------------------------------------------------------------
class Level(object):
    '''One level as the kernels see it: the local CSR pattern, the fp16
    weights ((nnz, 2) halves, or (nnz,) and `idrows` for the one-plane
    format), diag / dinv as (n, 2) floats, the Chebyshev interval.'''

    def __init__(self, rowptr, cols, diag_idx, a00, a11, one_plane=False):
        rp = numpy.asarray(rowptr, dtype=numpy.int64)
        n = len(rp) - 1
        self.rp, self.cols, self.n = rp, numpy.asarray(cols), n
        self.lens = numpy.diff(rp)
        self.nnz = int(rp[-1])
        self.row_of = numpy.repeat(numpy.arange(n), self.lens)
        self.diag_idx = numpy.asarray(diag_idx, dtype=numpy.int64)
        p = SimpleNamespace(n=n, nnz=self.nnz, rowptr=rp, cols=self.cols,
                            row_of=self.row_of, diag_idx=self.diag_idx,
                            a00=a00, a11=a11)
        if one_plane:
            self.w, self.idrows, self.diag, self.dinv = pmg_one_plane(p)
        else:
            self.w, self.diag, self.dinv = pmg_two_planes(p)
            self.idrows = None
        self.ulp = None
        self.lo = self.hi = None

    def w_f32(self, mut=()):
        w = self.w.astype(numpy.float32)
        if 'weight_ulp' in mut:
            # (component 0 only; one step towards zero on the fp16 grid)
            k = (self.ulp, 0) if w.ndim == 2 else self.ulp
            one = numpy.array([w[k]], dtype=numpy.float16)
            w[k] = (one.view(numpy.uint16) - 1).view(numpy.float16)[0]
        return w

    def interval(self, ratio):
        '''[lam / ratio, 1.1 lam] with lam from a power iteration on the fp16
        operator (the host tests; a device brings its own).'''
        v = numpy.random.RandomState(5).standard_normal((self.n, 2))
        lam = 0.0
        for _ in range(30):
            v = tile_product(self.rp, self.cols, self.w, v,
                             idrows=self.idrows)[0]
            lam = numpy.linalg.norm(v, axis=0)
            v = v / lam
        self.lo, self.hi = float(lam.max()) / ratio, SAFETY * float(lam.max())


def make_mesh(name):
    from flow_amd import fem
    if name == 'rect':
        return fem.RectangleMesh(fem.Point(-1.0, -0.5), fem.Point(1.5, 1.0), 7,
                                 5, 'left/right')
    assert name == 'karman'
    return fem.karman_channel(30, 10, fitted=True)


def _planes(lay, seed, bc, scalar):
    '''Four planes (kind 2) over the layout's pattern: diagonal 1 + U(0, 1),
    off-diagonals U(-1, 1) / row length, another seed for each of the diagonal
    blocks 0 and 3, large garbage in 1 and 2, identity rows on the Dirichlet
    dofs bc (n, 2).  scalar: one plane (kind 0), the rows bc[:, 0].'''
    rp = lay.pattern('rowptr').astype(numpy.int64)
    di = lay.pattern('diag_idx').astype(numpy.int64)
    lens = numpy.diff(rp)
    row_of = numpy.repeat(numpy.arange(lay.N), lens)
    out = []
    for plane in range(1 if scalar else 4):
        rng = numpy.random.RandomState(seed + plane)
        if plane in (1, 2):
            out.append(1.0e6 * rng.standard_normal(lay.nnz))
            continue
        a = rng.uniform(-1.0, 1.0, size=lay.nnz) / lens[row_of]
        a[di] = 1.0 + rng.uniform(size=lay.N)
        rows = bc[:, 0 if plane == 0 else 1] != 0
        a[rows[row_of]] = 0.0
        a[di[rows]] = 1.0
        out.append(a)
    return out


class Problem(object):
    '''Real layouts of a small mesh with synthetic matrices on them, as the
    model needs them and as a device is given them.

    mesh: 'rect' (165 P2 / 48 P1 dofs, restriction lists of 3 .. 9 entries,
    none of 8) or 'karman' (1272 / 340 dofs, lists of 3 .. 8, exactly one of
    8); one_plane: the ONE_PLANE format; scalar: a scalar P2 space with kind-0
    matrices; block = (g, world): the diagonal block of strip g.'''

    def __init__(self, mesh='rect', one_plane=False, scalar=False, block=None,
                 seed=100):
        from flow_amd.fem.pmg import transfer_tables, local_transfer_tables
        from flow_amd.fem.space import scalar_layout
        self.name = mesh
        self.mesh = make_mesh(mesh)
        self.scalar, self.one_plane, self.block = scalar, one_plane, block
        lay2 = self.lay2 = scalar_layout(self.mesh, 2)
        lay1 = self.lay1 = scalar_layout(self.mesh, 1)
        N, N1 = lay2.N, lay1.N
        # Dirichlet dofs: a seeded tenth of the vertex dofs and of the edge
        # dofs in both components, one vertex dof in component 0 only and one
        # edge dof in component 1 only
        rng = numpy.random.RandomState(seed)
        vd = rng.permutation(lay2.vertex_dofs.astype(numpy.int64))
        ed = rng.permutation(lay2.edge_dofs.astype(numpy.int64))
        both = numpy.concatenate([vd[:max(3, len(vd) // 10)],
                                  ed[:max(3, len(ed) // 10)]])
        bc = numpy.zeros((N, 2), dtype=numpy.uint8)
        bc[both] = 1
        if not scalar:
            bc[vd[-1], 0] = 1
            bc[ed[-1], 1] = 1
            self.single = (int(vd[-1]), int(ed[-1]))
            self.bc_dofs = numpy.sort(numpy.concatenate(
                [numpy.nonzero(bc[:, 0])[0], N + numpy.nonzero(bc[:, 1])[0]]))
        else:
            self.bc_dofs = numpy.sort(both)
        bcc = bc[lay2.vertex_dofs.astype(numpy.int64)]
        self.planes = _planes(lay2, seed + 10, bc, scalar)
        self.planes1 = _planes(lay1, seed + 20, bcc, scalar)
        blocks = (self.planes[0], self.planes[-1]), \
            (self.planes1[0], self.planes1[-1])
        if block is None:
            self.rows, self.vrows = None, None
            lv = [Level(lay.pattern('rowptr'), lay.pattern('cols'),
                        lay.pattern('diag_idx'), a[0], a[1], one_plane)
                  for lay, a in zip((lay2, lay1), blocks)]
            ends, rptr, rsrc = transfer_tables(lay2)
            self.keep = (None, None)
        else:
            from flow_amd import parallel
            g, world = block
            st = parallel.Strips(self.mesh, world)
            self.rows = st.blocks(lay2).rows(g)
            self.vrows = st.blocks(lay1).rows(g)
            lv, keeps = [], []
            for lay, a, rows in zip((lay2, lay1), blocks,
                                    (self.rows, self.vrows)):
                loc, keep = _local_pattern(lay, rows)
                k0, k1 = loc['k']
                lv.append(Level(
                    loc['rowptr'], loc['cols'], loc['diag_idx'],
                    numpy.where(keep, a[0][k0:k1], 0.0),
                    numpy.where(keep, a[1][k0:k1], 0.0), one_plane))
                keeps.append(keep)
            self.keep = tuple(keeps)
            ends, rptr, rsrc = local_transfer_tables(lay2, self.rows,
                                                     self.vrows)
            (r0, r1), (v0, v1) = self.rows, self.vrows
            bc, bcc = bc[r0:r1], bcc[v0:v1]
        self.fine, self.coarse = lv
        self.n, self.n1 = self.fine.n, self.coarse.n
        self.ends, self.rptr, self.rsrc = ends.reshape(-1, 2), rptr, rsrc
        self.bc, self.bcc = bc, bcc
        self.fine.interval(RATIO_FINE)
        self.coarse.interval(RATIO_COARSE)
        # the weight that 'weight_ulp' moves: the largest off-diagonal one of
        # a free row in the middle of the fine level
        F = self.fine
        free = numpy.nonzero((self.bc == 0).all(axis=1))[0]
        row = int(free[len(free) // 2])
        a, b = int(F.rp[row]), int(F.rp[row + 1])
        wabs = numpy.abs(F.w[a:b].astype(numpy.float64)).reshape(b - a, -1)[:, 0]
        wabs[F.diag_idx[row] - a] = 0.0
        F.ulp = a + int(numpy.argmax(wabs))

    def list_lengths(self):
        return numpy.diff(numpy.asarray(self.rptr, dtype=numpy.int64))

    def rhs(self, trial, seed=7):
        '''r: standard normal; trial 1: zero on the Dirichlet rows (what the
        Newton systems hand the cycle).  2n entries; in scalar mode the second
        half is NaN -- nothing may read it.'''
        rng = numpy.random.RandomState(seed + trial)
        r2 = rng.standard_normal((self.n, 2))
        if trial == 1:
            r2[self.bc != 0] = 0.0
        if self.scalar:
            return numpy.concatenate([r2[:, 0], numpy.full(self.n, numpy.nan)])
        return numpy.concatenate([r2[:, 0], r2[:, 1]])


def _local_pattern(lay, rows):
    '''The local CSR of the diagonal block of `rows`, as pmg._Level builds it:
    couplings that leave the block keep their place with column = own row and
    keep = False.'''
    r0, r1 = rows
    rp = lay.pattern('rowptr').astype(numpy.int64)
    k0, k1 = int(rp[r0]), int(rp[r1])
    cols = lay.pattern('cols')[k0:k1].astype(numpy.int64)
    row_of = numpy.repeat(numpy.arange(r0, r1), numpy.diff(rp[r0:r1 + 1]))
    keep = (cols >= r0) & (cols < r1)
    return dict(rowptr=rp[r0:r1 + 1] - k0,
                cols=numpy.where(keep, cols - r0, row_of - r0),
                diag_idx=lay.pattern('diag_idx')[r0:r1].astype(numpy.int64) - k0,
                k=(k0, k1)), keep


def standin_runs(prob, r, configs, mut=()):
    '''{config: run} of the fp32 stand-in, as a device would be observed.'''
    runs = {}
    # ONE work buffer for all runs, as on a device: what a run does not write
    # is left over from the setup (here: noise) or from the run before
    work = numpy.random.RandomState(9).standard_normal(
        work_size(prob.n, prob.n1)).astype(numpy.float32)
    work[-2:] = 0.0
    for cfg in configs:
        z = numpy.full(2 * prob.n, SENTINEL)
        work = cycle_f32(cfg, prob, r, z, work=work, mut=mut)
        runs[cfg] = observe(work, z, prob.n, prob.n1, prob.scalar)
    return runs
