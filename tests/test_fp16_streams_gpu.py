# -*- coding: utf-8 -*-
'''
The fp16 CSR-stream products row by row against an exact model (-m gpu):
fp16_tile_row_sum (flow_amd/csrc/csr_stream16.h) behind the mass solver's plain
and packed streams and the three p-multigrid level formats, on synthetic
patterns that put tiles at every alignment residue, at the cap of 2044
nonzeros, around a group of xcd_tile and at column spans of 65535 / 65536
(tests/fp16_stream_reference.py; what the comparison can and cannot see:
tests/test_fp16_streams_host.py).

(a) what the setup kernels write, bit for bit; (b) every launch of one mass
correction; (c) one product of a level through the power iteration.  The
device structs are built by the product's own MassSolver and _Level over a
stub layout: slack and alignment are the product's rules.  Every row is
compared, with the bound (len + 4) 2^-24 (sum |w| |g| + |epilogue operands|).
'''
import functools

import numpy
import pytest

import fp16_stream_reference as ref

pytestmark = pytest.mark.gpu


def _dev(a):
    from flow_amd import device
    return device.to_device(numpy.ascontiguousarray(a))


def _host(t):
    from flow_amd import device
    return device.to_host(t).numpy()


def _bits(a):
    a = numpy.ascontiguousarray(a)
    return a.view({2: numpy.uint16, 4: numpy.uint32}[a.dtype.itemsize])


@functools.lru_cache(maxsize=None)
def _layout(name):
    return ref.StubLayout(ref.pattern(name))


def _overflows(name):
    return name == 'wide_overflow'


# -- (a) the setup kernels --------------------------------------------------------
@pytest.mark.parametrize('name', ref.PATTERNS)
def test_mass_pack_kernels_bit_for_bit(hip, name):
    from flow_amd.fem import mass as fmass, ops
    p, lay = ref.pattern(name), _layout(name)
    A = ops.Matrix(lay, 0, _dev(p.vals))
    solver = fmass.MassSolver(A, _dev(1.0 / p.vals[p.diag_idx]), steps=3)
    w = ref.mass_weights(p)
    v16 = _host(solver.vals16)
    assert numpy.array_equal(_bits(v16[:p.nnz]), _bits(w))
    assert not v16[p.nnz:].any()                  # nothing behind the last one
    cbase, off, fits = ref.tile_bases(p)
    assert fits != _overflows(name)
    if not fits:
        # an offset of 65536: the flag is raised, the plain stream stays
        assert solver.packed16 is None
        return
    pk, cb = solver.packed16
    assert numpy.array_equal(_host(cb), cbase)
    words = _host(pk)
    assert numpy.array_equal(_bits(words[:p.nnz]), ref.packed_words(w, off))
    assert not words[p.nnz:].any()


def _jacobian(p, lay):
    '''Kind 2 (four planes); the levels take the diagonal blocks 0 and 3.'''
    import torch
    from flow_amd import device
    from flow_amd.fem import ops
    J = ops.Matrix(lay, 2)
    J.plane(0).copy_(torch.from_numpy(p.a00))
    J.plane(3).copy_(torch.from_numpy(p.a11))
    device.synchronize()
    return J


def _level(p, lay, fmt, monkeypatch):
    from flow_amd.fem import pmg as fpmg
    monkeypatch.setattr(fpmg, 'COLS16', fmt != 'cols32')
    monkeypatch.setattr(fpmg, 'ONE_PLANE', fmt == 'one_plane')
    level = fpmg._Level(lay)
    level.pack(_jacobian(p, lay))
    return level


@pytest.mark.parametrize('name', ref.PATTERNS)
def test_pmg_pack_kernels_bit_for_bit(hip, name, monkeypatch):
    p, lay = ref.pattern(name), _layout(name)
    n, nnz = p.n, p.nnz
    cbase, off, fits = ref.tile_bases(p)
    assert fits != _overflows(name)
    # half2 values, diag, dinv; 16-bit offsets and the tiles' base columns
    level = _level(p, lay, 'cols16', monkeypatch)
    w, diag, dinv = ref.pmg_two_planes(p)
    vals = _host(level.vals)
    assert numpy.array_equal(_bits(vals[:2 * nnz]).reshape(nnz, 2), _bits(w))
    assert not vals[2 * nnz:].any()
    assert numpy.array_equal(_bits(_host(level.diag)).reshape(n, 2), _bits(diag))
    assert numpy.array_equal(_bits(_host(level.dinv)).reshape(n, 2), _bits(dinv))
    if fits:
        c16, cb = level._cols16
        assert numpy.array_equal(_host(cb), cbase)
        assert numpy.array_equal(_bits(_host(c16))[:nnz], off)
    else:
        assert level._cols16 is None
    # ONE plane: packed words, identity-row flags, the mean diagonal
    level = _level(p, lay, 'one_plane', monkeypatch)
    if not fits:
        assert level._cols16 is None and level._packed is None
        return
    w1, idr, diag, dinv = ref.pmg_one_plane(p)
    pk, flags = level._packed
    assert numpy.array_equal(ref.blocked(_host(flags), n), idr)
    words = _host(pk)
    assert numpy.array_equal(_bits(words[:nnz]), ref.packed_words(w1, off))
    assert not words[nnz:].any()
    assert numpy.array_equal(_bits(_host(level.diag)).reshape(n, 2), _bits(diag))
    assert numpy.array_equal(_bits(_host(level.dinv)).reshape(n, 2), _bits(dinv))


# -- (b) one mass correction, launch by launch ---------------------------------------
def _correction(p, lay, kind, packed, steps, g, dinv):
    '''One correction from x = 0 with `steps` Chebyshev steps: (work16 as
    (5, n, ncomp), z as (n, ncomp), (lam_min, lam_max)).'''
    from flow_amd import _hip
    from flow_amd.fem import mass as fmass, ops
    ncomp = 2 if kind == 4 else 1
    n = p.n
    mask = _dev(p.rowmask) if kind == 4 else None
    A = ops.Matrix(lay, kind, _dev(p.vals), rowmask=mask)
    solver = fmass.MassSolver(A, _dev(dinv), steps=steps, packed=packed)
    solver.guard = False
    if packed and _overflows(p.name):
        assert solver.packed16 is None            # the plain stream is taken
    else:
        assert (solver.packed16 is not None) == packed
    x = _dev(numpy.full(ncomp * n, 7.0))
    xbase = _dev(numpy.zeros(ncomp * n))
    # (not a mass matrix: one correction does not meet rtol = 0)
    with pytest.raises(_hip.NotConverged):
        solver.solve_increment(_dev(g), xbase, x, rtol=0.0, maxit=1)
    work = _host(solver.work16)[:5 * ncomp * n].reshape(5, n, ncomp)
    z = _host(x).reshape(ncomp, n).T
    return work, z, (solver.struct.lam_min, solver.struct.lam_max)


@pytest.mark.parametrize('packed', [False, True], ids=['plain', 'packed'])
@pytest.mark.parametrize('kind', [0, 4], ids=['scalar', 'pair'])
@pytest.mark.parametrize('name', ref.PATTERNS)
def test_mass_products_row_by_row(hip, name, kind, packed):
    p, lay = ref.pattern(name), _layout(name)
    rng = numpy.random.RandomState(40 + kind)
    n, ncomp = p.n, (2 if kind == 4 else 1)
    rp, cols = p.rowptr, p.cols
    w = ref.mass_weights(p)
    dinv = numpy.tile(1.0 / p.vals[p.diag_idx], ncomp)
    mask = None
    if kind == 4:
        dinv[p.rowmask == 0] = 1.0
        mask = ref.blocked(p.rowmask, n)
    g = rng.standard_normal(ncomp * n)
    tag = 'mass %s %s %s ' % (name, 'pair' if kind == 4 else 'scalar',
                              'packed' if packed else 'plain')
    worst = []

    def check(got, lines):
        for what, want, bound in lines:
            worst.append(ref.assert_rows(
                got[what], want.reshape(n, ncomp), bound.reshape(n, ncomp),
                tag + what))

    def shaped(a):
        return a if ncomp == 2 else a[:, 0]

    # steps = 3: MODE 0, MODE 2
    work, z, (lo, hi) = _correction(p, lay, kind, packed, 3, g, dinv)
    c0, c = ref.cheb_coefficients(lo, hi, 3)
    rho0, rho1, d1, acc1 = work[0], work[1], work[2], work[4]
    assert numpy.array_equal(
        _bits(rho0), _bits(numpy.float32(dinv * g).reshape(ncomp, n).T))
    check(dict(rho=rho1, d=d1, acc=acc1), ref.mass_mode0(
        rp, cols, w, mask, shaped(rho0), (c0, c[0]), shaped(rho1), shaped(d1)))
    check(dict(z=z), ref.mass_step(rp, cols, w, mask, shaped(d1), shaped(rho1),
                                   shaped(acc1), c[1]))
    # steps = 4: the same MODE 0, then MODE 1 and MODE 2
    work, z, _ = _correction(p, lay, kind, packed, 4, g, dinv)
    rho2, d2, acc2 = work[1], work[3], work[4]
    assert numpy.array_equal(_bits(work[0]), _bits(rho0))
    assert numpy.array_equal(_bits(work[2]), _bits(d1))
    check(dict(rho=rho2, d=d2, acc=acc2), ref.mass_step(
        rp, cols, w, mask, shaped(d1), shaped(rho1), shaped(acc1), c[1],
        shaped(rho2), shaped(d2)))
    check(dict(z=z), ref.mass_step(rp, cols, w, mask, shaped(d2), shaped(rho2),
                                   shaped(acc2), c[2]))
    print('RATIO %s%.3g' % (tag, max(worst)))


# -- (c) one product of a p-multigrid level -------------------------------------------
@pytest.mark.parametrize('fmt', ['cols32', 'cols16', 'one_plane'])
@pytest.mark.parametrize('name', ref.PATTERNS)
def test_pmg_level_products_row_by_row(hip, name, fmt, monkeypatch):
    '''flow_pmg_lambda_max, two passes from v0: it leaves w1 = -(A~ v0) /
    |A~ v0| in work[2n:4n] (one product, row by row) and returns |A~ w1| (the
    second product, in norm).'''
    import torch
    from flow_amd import device
    p, lay = ref.pattern(name), _layout(name)
    n = p.n
    monkeypatch.delenv('FLOW_AMD_PMG_COLD_POWER', raising=False)
    level = _level(p, lay, fmt, monkeypatch)
    fits = not _overflows(name)
    assert (level._cols16 is not None) == (fmt != 'cols32' and fits)
    assert (level._packed is not None) == (fmt == 'one_plane' and fits)
    if level._packed is not None:
        w, idr = ref.pmg_one_plane(p)[:2]
    else:
        w, idr = ref.pmg_two_planes(p)[0], None
    v0 = numpy.random.RandomState(50).standard_normal((n, 2)).astype(
        numpy.float32)
    level._eigvec = _dev(v0.reshape(-1))        # the start of a warm call
    work = torch.zeros(6 * n, dtype=torch.float32, device=device.get())
    lam = level.lambda_max(work, iterations=2, warm_iterations=2)
    w1 = _host(work)[2 * n:4 * n].reshape(n, 2)
    want, bound = ref.power_pass(p.rowptr, p.cols, w, v0, idrows=idr)
    tag = 'pmg %s %s w1' % (name, fmt)
    worst = ref.assert_rows(w1, want, bound, tag)
    lam_ref, tol = ref.norm_of_product(p.rowptr, p.cols, w, w1, idrows=idr)
    print('RATIO %s %.3g ; | |A w1| - model | / tolerance = %.3g'
          % (tag, worst, abs(lam - lam_ref) / tol))
    assert abs(lam - lam_ref) <= tol, (lam, lam_ref, tol)
