# -*- coding: utf-8 -*-
'''
The row-by-row check of the fp16 CSR-stream products (tests/
test_fp16_streams_gpu.py) without a GPU: the synthetic patterns really hold the
edges they advertise, the model restates the setup kernels' tables
consistently, and the comparator CAN fail -- it accepts the model evaluated in
fp32 the way the kernel evaluates it and rejects that result with one seeded
defect each: a dropped last nonzero of a tile, a first nonzero taken from the
alignment slack, tiles permuted without inverting xcd_tile, a 16-bit offset
wrapped at 65536, a weight one fp16 ulp off on a row of one entry, an identity
row not applied.
'''
import numpy
import pytest

import access_model
import fp16_stream_reference as ref

NORMAL16 = 2.0**-14


def _vector(p, seed, ncomp=1):
    rng = numpy.random.RandomState(seed)
    shape = (p.n,) if ncomp == 1 else (p.n, 2)
    return rng.standard_normal(shape).astype(numpy.float32)


# -- the patterns ----------------------------------------------------------------
def test_every_advertised_edge_occurs():
    p = ref.pattern('residues')
    assert p.residues() == {0, 1, 2, 3}
    assert p.lens.min() == 1 and p.lens.max() > 8
    p = ref.pattern('full')
    k0, k1 = p.tile_k()
    rows = numpy.diff(p.rowblocks)
    full = (k1 - k0) == ref.TILE_NNZ
    # one row of 2044 and 256 rows of 7 / 8, each at k0 % 4 == 0 and == 3
    for nrows in (1, 256):
        assert set(k0[full & (rows == nrows)] % 4) == {0, 3}, nrows
    assert (p.tile_hi() == 2047).sum() == 2 and p.tile_hi().max() == 2047
    assert ((rows == 256) & ((k1 - k0) == 256)).any()      # 256 rows of one entry
    for nt in (1, 7, 9, 523):
        p = ref.pattern('tiles%d' % nt)
        rows = numpy.diff(p.rowblocks)
        assert len(rows) == nt and p.n < 5000
        assert nt == 1 or rows[-1] < rows[0]
    assert p.residues() == {0, 1, 2, 3}                    # (of the 523 tiles)
    p = ref.pattern('wide')
    assert p.n >= 65537 and p.tile_spans().max() == 65535
    assert ref.tile_bases(p)[2]
    for name in ('wide', 'wide_overflow'):
        # the entries at both ends of the span carry a weight in every format
        p = ref.pattern(name)
        cbase, off, _ = ref.tile_bases(p)
        k0, k1 = p.tile_k()
        t = int(numpy.argmax(p.tile_spans()))
        assert cbase[t] == ref.WIDE_CMIN > 0
        ends = k0[t] + numpy.array([numpy.argmin(off[k0[t]:k1[t]]),
                                    numpy.argmax(off[k0[t]:k1[t]])])
        for w in (ref.mass_weights(p), ref.pmg_two_planes(p)[0],
                  ref.pmg_one_plane(p)[0]):
            assert (numpy.abs(w[ends].astype(float)) > 0.3).all()
    p = ref.pattern('wide_overflow')
    assert p.n >= 65537 and p.tile_spans().max() == 65536
    assert (p.tile_spans() > 65535).sum() == 1 and not ref.tile_bases(p)[2]


@pytest.mark.parametrize('name', ref.PATTERNS)
def test_patterns_are_what_the_kernels_may_be_given(name):
    '''Tiles of at most 256 rows and 2044 nonzeros, columns inside [0, n): and
    with them every index the tile routine forms lies inside the arrays the
    product allocates (the access model of the routine, access_model.py).'''
    p = ref.pattern(name)
    ref.check_preconditions(p)
    cols = numpy.concatenate([p.cols, numpy.zeros(4, dtype=p.cols.dtype)])
    lo, hi, last = access_model.quad_tile_accesses(p.rowptr, cols, p.rowblocks)
    assert lo.min() >= 0 and hi.max() < p.n and last.max() < p.nnz + 4
    # values: every class of scaled entry occurs, none overflows fp16
    off = numpy.ones(p.nnz, dtype=bool)
    off[p.diag_idx] = False
    for w in (ref.mass_weights(p), ref.pmg_two_planes(p)[0],
              ref.pmg_one_plane(p)[0]):
        a = numpy.abs(w.astype(numpy.float64))
        assert numpy.isfinite(a).all() and a.max() <= 4.0
        # (the one-plane level zeroes what touches an identity row)
        if p.nnz > 100 and (w.ndim == 2 or w is not ref.pmg_one_plane(p)[0]):
            assert (a == 0.0).any() and ((a > 0.0) & (a < NORMAL16)).any()
            assert (a[off] >= NORMAL16).any() and a[off].max() > 0.25
    assert not numpy.array_equal(p.a00, p.a11)
    if p.n > 50:
        idr = ref.pmg_idrows(p)[p.lens > 1]
        for flags in ((1, 0), (0, 1), (1, 1), (0, 0)):
            assert ((idr[:, 0] == flags[0]) & (idr[:, 1] == flags[1])).any(), flags
        assert 0 < p.rowmask.sum() < 2 * p.n


def test_xcd_tile_is_a_bijection_with_the_runs_of_common_h():
    for nwg in (1, 7, 9, 511, 512, 523, 1024 + 13):
        t = [ref.xcd_tile(b, nwg) for b in range(nwg)]
        assert sorted(t) == list(range(nwg))
    # 523 = a full group (runs of 64 per XCD) + 11 tiles: runs of 2, 2, 2, 1 ...
    t = [ref.xcd_tile(b, 523) for b in range(523)]
    assert t[:9] == [0, 64, 128, 192, 256, 320, 384, 448, 1]
    assert t[512:523] == [512, 514, 516, 518, 519, 520, 521, 522, 513, 515, 517]


def test_tables_agree_with_the_access_models_restatement():
    '''cbase / offsets: two restatements written apart (access_model.py) agree;
    the packed word splits back into its halves.'''
    for name in ('residues', 'tiles523', 'wide', 'wide_overflow'):
        p = ref.pattern(name)
        cbase, off, fits = ref.tile_bases(p)
        cb2, off2, fits2 = access_model.cols16_tables(p.rowptr, p.cols, p.rowblocks)
        assert numpy.array_equal(cbase, cb2) and numpy.array_equal(off, off2)
        assert fits == fits2 == (name != 'wide_overflow')
        if fits:
            w = ref.mass_weights(p)
            words = ref.packed_words(w, off)
            assert words.dtype == numpy.uint32
            assert numpy.array_equal(words >> 16, off)
            assert numpy.array_equal((words & 0xffff).astype(numpy.uint16),
                                     w.view(numpy.uint16))


def test_roundings_and_coefficients():
    # ONE rounding double -> half: 1 + 2^-11 + 2^-30 lies above the tie and
    # rounds up; through float it would first fall ON the tie (1 + 2^-11) and
    # then to even (1.0)
    v = numpy.array([1.0 + 2.0**-11 + 2.0**-30])
    assert ref.round16(v, 1.0)[0] == numpy.float16(1.0 + 2.0**-10)
    assert ref.round16_via_float(v, 1.0)[0] == numpy.float16(1.0)
    # ... which the larger patterns meet (2^-13 of all entries): the bit-for-
    # bit tests of the setup kernels tell the two apart
    p = ref.pattern('wide')
    d = p.vals[p.diag_idx][p.row_of]
    differ = ref.round16(p.vals, d) != ref.round16_via_float(p.vals, d)
    assert 0 < differ.sum() < 40
    assert ref.round16(numpy.array([3e-6]), 1.0)[0] != 0        # subnormal kept
    # Cheb (csr_stream16.h) against the recurrence written out
    lo, hi = 0.49, 2.02
    c0, steps = ref.cheb_coefficients(lo, hi, 3)
    theta, delta = 0.5 * (hi + lo), 0.5 * (hi - lo)
    sigma = theta / delta
    assert c0 == numpy.float32(1.0 / theta) and c0.dtype == numpy.float32
    r0 = 1.0 / sigma
    r1 = 1.0 / (2.0 * sigma - r0)
    r2 = 1.0 / (2.0 * sigma - r1)
    assert steps[0] == (numpy.float32(r1 * r0), numpy.float32(2.0 * r1 / delta))
    assert steps[1] == (numpy.float32(r2 * r1), numpy.float32(2.0 * r2 / delta))


def test_the_exact_model_against_a_dense_product():
    p = ref.pattern('residues')
    rng = numpy.random.RandomState(3)
    w = ref.pmg_two_planes(p)[0].astype(numpy.float64)
    g = rng.standard_normal((p.n, 2))
    idr = ref.pmg_idrows(p)
    s, sabs = ref.tile_product(p.rowptr, p.cols, w, g, idrows=idr)
    for a in range(2):
        A = numpy.zeros((p.n, p.n))
        A[p.row_of, p.cols] = w[:, a]
        want = numpy.where(idr[:, a] != 0, g[:, a], A.dot(g[:, a]))
        assert numpy.allclose(s[:, a], want, rtol=1e-13, atol=1e-15)
        wabs = numpy.where(idr[:, a] != 0, abs(g[:, a]),
                           abs(A).dot(abs(g[:, a])))
        assert numpy.allclose(sabs[:, a], wabs, rtol=1e-13, atol=1e-15)
    # scalar vector, one weight per nonzero, mask (0 = identity)
    mask = p.rowmask[:p.n]
    s1, _ = ref.tile_product(p.rowptr, p.cols, w[:, 0], g[:, 0], mask=mask)
    A = numpy.zeros((p.n, p.n))
    A[p.row_of, p.cols] = w[:, 0]
    assert numpy.allclose(s1, numpy.where(mask == 0, g[:, 0], A.dot(g[:, 0])),
                          rtol=1e-13, atol=1e-15)


# -- the comparator accepts the kernel's arithmetic ---------------------------------
@pytest.mark.parametrize('name', ref.PATTERNS)
def test_comparator_accepts_the_model_in_fp32(name):
    p = ref.pattern(name)
    rp, cols, lens = p.rowptr, p.cols, p.lens
    w = ref.mass_weights(p)
    c0, steps = ref.cheb_coefficients(0.49, 2.02, 3)
    for ncomp in (1, 2):
        mask = None if ncomp == 1 else ref.blocked(p.rowmask, p.n)
        rho0 = _vector(p, 11, ncomp)
        m0 = ref.mass_mode0_f32(rp, cols, w, mask, rho0, (c0, steps[0]))
        for what, want, bound in ref.mass_mode0(
                rp, cols, w, mask, rho0, (c0, steps[0]), m0['rho'], m0['d']):
            r = ref.assert_rows(m0[what], want, bound, 'host %s mode0 %s' %
                                (name, what))
            assert r < 0.5
        m1 = ref.mass_step_f32(rp, cols, w, mask, m0['d'], m0['rho'], m0['acc'],
                               steps[1])
        for what, want, bound in ref.mass_step(
                rp, cols, w, mask, m0['d'], m0['rho'], m0['acc'], steps[1],
                m1['rho'], m1['d']):
            ref.assert_rows(m1[what], want, bound, 'host %s mode1 %s' %
                            (name, what))
        (what, want, bound), = ref.mass_step(
            rp, cols, w, mask, m0['d'], m0['rho'], m0['acc'], steps[1])
        ref.assert_rows(m1['z'], want, bound, 'host %s mode2 z' % name)
    v0 = _vector(p, 12, 2)
    for w2, idr in ((ref.pmg_two_planes(p)[0], None),
                    (ref.pmg_one_plane(p)[0], ref.pmg_idrows(p))):
        got = ref.power_pass_f32(rp, cols, w2, v0, idrows=idr)
        want, bound = ref.power_pass(rp, cols, w2, v0, idrows=idr)
        assert ref.assert_rows(got, want, bound, 'host %s w1' % name) < 0.5
        lam, tol = ref.norm_of_product(rp, cols, w2, got, idrows=idr)
        got2 = ref.tile_product_f32(rp, cols, w2, got, idrows=idr)
        assert abs(numpy.linalg.norm(got2.astype(numpy.float64)) - lam) <= tol
    assert lens.max() == numpy.diff(rp).max()


# -- and rejects every seeded defect ---------------------------------------------
def _row_f32(w, g, cols, a, b):
    '''One row the way a lane sums it: fp32, in the order of the nonzeros.'''
    s = numpy.zeros(g.shape[1:], dtype=numpy.float32)
    for k in range(a, b):
        s = s + numpy.float32(w[k]) * g[cols[k]]
    return s


def _rejected(p, w, g, got, idrows=None, mask=None):
    '''Both comparisons of the GPU tests -- the plain row sums and the scaled
    vector of the power iteration (the widest bound) -- reject `got`; returns
    the row that is worst off.'''
    want, sabs = ref.tile_product(p.rowptr, p.cols, w, g, idrows=idrows,
                                  mask=mask)
    bound = ref.row_bound(p.lens, sabs)
    worst, at = ref.worst_ratio(got, want, bound)
    with pytest.raises(AssertionError):
        ref.assert_rows(got, want, bound, 'seeded defect')
    if mask is None:
        nrm = numpy.linalg.norm(got.astype(numpy.float64))
        w1 = (numpy.float32(0.0) - got) * numpy.float32(1.0 / nrm)
        want1, bound1 = ref.power_pass(p.rowptr, p.cols, w, g, idrows=idrows)
        with pytest.raises(AssertionError):
            ref.assert_rows(w1, want1, bound1, 'seeded defect, scaled')
    assert worst > 100.0, worst
    return at[0]


def _one_row_defects(name, change):
    '''The clean fp32 result with one row redone after `change(p, w, cols, tile, g)
    -> row` edited copies of the weights / columns: for every tile where the
    defect is material (change returns None otherwise).'''
    p = ref.pattern(name)
    w = ref.mass_weights(p).astype(numpy.float32)
    g = _vector(p, 21)
    clean = ref.tile_product_f32(p.rowptr, p.cols, w, g)
    want, sabs = ref.tile_product(p.rowptr, p.cols, w, g)
    ref.assert_rows(clean, want, ref.row_bound(p.lens, sabs), 'clean ' + name)
    hit = []
    for tile in range(len(p.rowblocks) - 1):
        w2, c2 = w.copy(), p.cols.copy()
        row = change(p, w2, c2, tile, g)
        if row is None:
            continue
        got = clean.copy()
        got[row] = _row_f32(w2, g, c2, p.rowptr[row], p.rowptr[row + 1])
        assert _rejected(p, w, g, got) == row
        hit.append(tile)
    return p, hit


@pytest.mark.parametrize('name', ['full', 'residues', 'tiles523'])
def test_rejects_a_dropped_last_nonzero_of_a_tile(name):
    def change(p, w, cols, tile, g):
        k = p.rowptr[p.rowblocks[tile + 1]] - 1
        # (material: the lost product is not tiny, its row not a long one)
        if abs(w[k] * g[cols[k]]) < 1e-3 or p.lens[p.row_of[k]] > 64:
            return None
        w[k] = 0.0
        return p.row_of[k]
    p, hit = _one_row_defects(name, change)
    assert len(hit) >= 0.3 * (len(p.rowblocks) - 1)
    if name == 'full':
        assert set(p.tile_hi()[hit]) >= {2047}


@pytest.mark.parametrize('name', ['full', 'residues', 'tiles523'])
def test_rejects_a_first_nonzero_taken_from_the_alignment_slack(name):
    def change(p, w, cols, tile, g):
        k = p.rowptr[p.rowblocks[tile]]
        if k % 4 == 0 or p.lens[p.row_of[k]] > 64 or \
                abs(w[k] * g[cols[k]] - w[k - 1] * g[cols[k - 1]]) < 1e-3:
            return None
        w[k], cols[k] = w[k - 1], cols[k - 1]
        return p.row_of[k]
    p, hit = _one_row_defects(name, change)
    k0, _ = p.tile_k()
    assert set(k0[hit] % 4) == {1, 2, 3}


@pytest.mark.parametrize('name', ['full', 'tiles523'])
def test_rejects_a_weight_one_ulp_off_on_a_row_of_one_entry(name):
    def change(p, w, cols, tile, g):
        r0, r1 = p.rowblocks[tile], p.rowblocks[tile + 1]
        rows = r0 + numpy.nonzero(p.lens[r0:r1] == 1)[0]
        if len(rows) == 0:
            return None
        k = p.rowptr[rows[-1]]
        bits = numpy.array([w[k]], dtype=numpy.float16).view(numpy.uint16)
        w[k] = (bits - 1).view(numpy.float16)[0]       # 1 - 2^-11
        return rows[-1]
    p, hit = _one_row_defects(name, change)
    assert len(hit) >= 5


@pytest.mark.parametrize('name', ['tiles9', 'tiles523'])
def test_rejects_tiles_permuted_without_inverting_xcd_tile(name):
    '''Workgroup b works on tile xcd_tile(b) but takes the base column of the
    16-bit offsets from cbase[b].'''
    p = ref.pattern(name)
    nt = len(p.rowblocks) - 1
    cbase, off, fits = ref.tile_bases(p)
    assert fits
    k0, k1 = p.tile_k()
    wrong = numpy.empty(nt, dtype=numpy.int64)
    for b in range(nt):
        wrong[ref.xcd_tile(b, nt)] = cbase[b]
    assert (wrong != cbase).any()
    cols = numpy.clip(numpy.repeat(wrong, k1 - k0) + off, 0, p.n - 1)
    w = ref.pmg_two_planes(p)[0]
    g = _vector(p, 22, 2)
    got = ref.tile_product_f32(p.rowptr, cols, w, g)
    _rejected(p, w, g, got)


def test_rejects_a_16_bit_offset_wrapped_at_65536():
    p = ref.pattern('wide_overflow')
    cbase, off, fits = ref.tile_bases(p)
    assert not fits and (off == 65536).sum() == 1
    k0, k1 = p.tile_k()
    cols = numpy.repeat(cbase, k1 - k0) + (off & 0xffff)
    w = ref.pmg_two_planes(p)[0]
    g = _vector(p, 23, 2)
    got = ref.tile_product_f32(p.rowptr, cols, w, g)
    row = _rejected(p, w, g, got)
    assert row == p.row_of[numpy.nonzero(off == 65536)[0][0]]
    # the same pattern one column narrower wraps nothing
    q = ref.pattern('wide')
    assert (ref.tile_bases(q)[1] & 0xffff == ref.tile_bases(q)[1]).all()


@pytest.mark.parametrize('name', ['residues', 'full'])
def test_rejects_an_identity_row_not_applied(name):
    p = ref.pattern(name)
    g = _vector(p, 24, 2)
    # the one-plane level's flags (1 = identity) ...
    w, idr = ref.pmg_one_plane(p)[:2]
    clean = ref.tile_product_f32(p.rowptr, p.cols, w, g, idrows=idr)
    for a in range(2):
        rows = numpy.nonzero((idr[:, a] != 0) & (p.lens > 1))[0]
        flags = idr.copy()
        flags[rows[0], a] = 0
        got = ref.tile_product_f32(p.rowptr, p.cols, w, g, idrows=flags)
        assert (got != clean).sum() == 1
        assert _rejected(p, w, g, got, idrows=idr) == rows[0]
    # ... and the pair mass operator's mask (0 = identity)
    w = ref.mass_weights(p)
    mask = ref.blocked(p.rowmask, p.n)
    rows = numpy.nonzero((mask[:, 1] == 0) & (p.lens > 1))[0]
    m2 = mask.copy()
    m2[rows[0], 1] = 1
    got = ref.tile_product_f32(p.rowptr, p.cols, w, g, mask=m2)
    assert _rejected(p, w, g, got, mask=mask) == rows[0]
