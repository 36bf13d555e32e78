# -*- coding: utf-8 -*-
'''
The row-by-row check of the fp64 CSR-stream products (tests/
test_fp64_streams_gpu.py) without a GPU: the synthetic patterns really hold the
edges they are named after, the exact data is exact (every absolute row sum
below 2^53 on its dyadic grid), a numpy emulation of the tile as csr_stream.h
states it reproduces the integer model on every pattern -- and both
comparisons CAN fail: each seeded defect of that emulation (alignment slack
ignored, the trailing odd nonzero dropped, the last pair of LDS slots dropped
at hi = cap + 1, the neighbour tile's first nonzero added, an empty tile
returning the previous tile's sums, a partial group of xcd_tile that is not a
bijection) is caught bit for bit on exact data and by more than 1e6 times the
bound on random data, while the unmutated emulation stays below 1.
'''
import numpy
import pytest

import fp64_stream_reference as ref

CAPS = sorted(set([ref.tile_cap(0), ref.tile_cap(2)]))
ALL = ref.SQUARE + ref.RECT


def _partitions(p):
    out = [('hand', None)]
    if p.name in ref.RECT:
        out.append(('own', p.own_rowblocks()))
    return out


# -- the patterns ----------------------------------------------------------------------
@pytest.mark.parametrize('cap', CAPS)
@pytest.mark.parametrize('name', ALL)
def test_patterns_hold_the_edges_they_are_named_after(name, cap):
    p = ref.pattern(name, cap)
    for what, rb in _partitions(p):
        ref.check_preconditions(p, rb)
    assert p.n <= 5000
    if name == 'full':
        # one row of `cap` entries and 256 rows, at both parities; hi = cap + 1
        k0, k1 = p.tile_k()
        assert sorted(ref.tile_hi(p)[k1 - k0 == cap]) == [cap, cap, cap + 1,
                                                          cap + 1]
    if name == 'empty_tiles':
        for what, rb in _partitions(p):
            e = ref.empty_tiles(p, rb)
            assert e[0] == 0 and e[-1] == len(p.rowblocks if rb is None else rb) - 2


def test_tile_counts_around_a_group_of_xcd_tile():
    for nt in (1, 7, 9, 523):
        p = ref.square('tiles%d' % nt, CAPS[0])
        assert len(p.rowblocks) - 1 == nt
        t = [ref.xcd_tile(b, nt) for b in range(nt)]
        assert sorted(t) == list(range(nt))
        # the seeded mapping is NOT a bijection wherever the partial group has
        # a remainder
        m = [ref.xcd_tile_remainder_ignored(b, nt) for b in range(nt)]
        assert (sorted(m) == list(range(nt))) == (nt % 8 == 0 or nt == 1)
    # the library's own mapping, where it is built
    from flow_amd import _hip
    try:
        lib = _hip.load_library()
    except (OSError, _hip.HipError):
        return
    for nt in (1, 7, 9, 523):
        assert [lib.flow_xcd_tile_host(b, nt) for b in range(nt)] == \
            [ref.xcd_tile(b, nt) for b in range(nt)]


# -- the exact data is exact ----------------------------------------------------------------
@pytest.mark.parametrize('name', ref.SQUARE)
def test_exact_data_of_the_square_kernels_stays_below_2_53(name):
    p = ref.square(name, CAPS[-1])
    v, x = ref.exact_data(p, 5)
    assert numpy.abs(v).max() <= ref.EXACT_MAG and numpy.abs(x).max() <= ref.EXACT_MAG
    if p.nnz > 100:
        assert (v == 0).any() and (v > 0).any() and (v < 0).any()
        assert (x == 0).any() and (x > 0).any() and (x < 0).any()
    assert (v[:, p.diag_idx] != 0).all()
    assert (v[:, p.definite] != 0).all() and (x[p.cols[p.definite]] != 0).all()
    mask = ref.row_mask(p)
    for kind in (0, 1, 2, 4):
        got, sabs = ref.int_product(kind, p, v, x, mask if kind == 4 else None)
        top = ref.assert_exact(sabs, '%s kind %d' % (name, kind))
        # (the bound the issue reasons with: cap terms of 2^20, two per slot)
        assert top <= 2 * (p.cap + 1) * ref.EXACT_MAG**2 < 2**53
        assert (numpy.abs(got) <= sabs).all()
    # the mass residual dinv (b - A x): dinv a power of two, b an integer
    ref.assert_exact(sabs + ref.EXACT_MAG, name + ' residual', grid=4)


def test_exact_data_of_the_multigrid_cycle_stays_below_2_53():
    ops = ref.mg_operators(CAPS[0])
    assert set(ops['dinv_exp']) == {0, 1, 2, 3, 4}
    for key in ('Ah', 'Ps', 'R'):
        assert numpy.abs(ops[key][1]).max() == ref.MG_MAG
        p = ops[key][0]
        ref.check_preconditions(p, p.own_rowblocks())
        assert not numpy.array_equal(p.own_rowblocks(), p.rowblocks)
    from flow_amd.fem.space import csr_stream_rowblocks
    up = csr_stream_rowblocks([ops['Ps'][0].rowptr, ops['Ah'][0].rowptr],
                              nnz_per_block=CAPS[0])
    assert len(ref.empty_tiles(ops['Ps'][0], up)) >= 3
    ref.check_preconditions(ops['Ah'][0], up)
    for fused in (False, True):
        for identity in (True, False):
            m = ref.mg_model(ops, fused, identity)
            for stage, sabs in m['sabs'].items():
                top = ref.assert_exact(sabs, 'mg %s' % stage)
                assert top < 32 * 2**43          # (the issue's estimate)
            assert numpy.abs(m['z32']).max() < 2**53
    # both forms are the same cycle
    a, b = ref.mg_model(ops, False), ref.mg_model(ops, True)
    assert numpy.array_equal(a['z32'], b['z32'])
    assert numpy.array_equal(a['r1'], b['r1']) and a['r1'].any()
    # C fits the tiles, and has more in a row than R
    C = ref.mg_restriction(ops)
    assert numpy.diff(C.indptr).max() <= CAPS[0]
    assert C.nnz > ops['R'][0].nnz and numpy.abs(C.data).max() > ref.MG_MAG


def test_the_integer_model_against_a_dense_product():
    p = ref.square('parity', CAPS[0])
    v, x = ref.exact_data(p, 6)
    n = p.n
    D = [numpy.zeros((n, n), dtype=numpy.int64) for _ in range(4)]
    for a in range(4):
        D[a][p.row_of, p.cols] = v[a]
    x0, x1 = x[:n], x[n:]
    assert numpy.array_equal(ref.int_product(0, p, v, x)[0], D[0].dot(x0))
    assert numpy.array_equal(ref.int_product(1, p, v, x)[0],
                             numpy.concatenate([D[0].dot(x0), D[1].dot(x1)]))
    assert numpy.array_equal(
        ref.int_product(2, p, v, x)[0],
        numpy.concatenate([D[0].dot(x0) + D[1].dot(x1),
                           D[2].dot(x0) + D[3].dot(x1)]))
    mask = ref.row_mask(p)
    want = numpy.concatenate([D[0].dot(x0), D[0].dot(x1)])
    assert numpy.array_equal(ref.int_product(4, p, v, x, mask)[0],
                             numpy.where(mask == 0, x, want))
    assert 0.05 * 2 * n < (mask == 0).sum() < 0.3 * 2 * n
    # the random-data model: correctly rounded, so within half an ulp of a
    # sum in extended precision
    vr, xr = ref.random_data(p, 7)
    got, bound = ref.float_product(2, p, vr, xr)
    L = numpy.longdouble
    want = numpy.zeros(n, dtype=L)
    numpy.add.at(want, p.row_of, vr[0].astype(L) * xr[p.cols].astype(L)
                 + vr[1].astype(L) * xr[n + p.cols].astype(L))
    assert (numpy.abs(got[:n] - want) <= 2.0**-52 * numpy.abs(want) + 1e-300).all()
    assert (bound > 0).all()


# -- the emulation of the tile: accepted, and every seeded defect rejected --------------------
def _cases():
    for cap in CAPS[:1]:
        for name in ALL:
            p = ref.pattern(name, cap)
            for what, rb in _partitions(p):
                yield name, what, p, rb


def _exact(p):
    v, x = ref.exact_data(p, 8, planes=1, ncomp=1)
    want, sabs = ref.int_product(0, p, v, x)
    ref.assert_exact(sabs, p.name)
    return v[0], x, want


def _random(p):
    v, x = ref.random_data(p, 9, planes=1, ncomp=1)
    want, bound = ref.float_product(0, p, v, x)
    return v[0], x, want, bound


def test_the_emulation_reproduces_both_models_on_every_pattern():
    for name, what, p, rb in _cases():
        v, x, want = _exact(p)
        ref.assert_bits(ref.emulate(p, v, x, rb), want, '%s %s' % (name, what))
        v, x, want, bound = _random(p)
        worst = ref.assert_rows(ref.emulate(p, v, x, rb), want, bound,
                                'host fp64 %s %s' % (name, what))
        assert worst < 1.0


@pytest.mark.parametrize('mutant', ref.MUTANTS)
def test_every_seeded_defect_is_caught(mutant):
    caught = []
    for name, what, p, rb in _cases():
        v, x, want = _exact(p)
        got = ref.emulate(p, v, x, rb, mutant)
        try:
            ref.assert_bits(got, want, name)
            continue
        except AssertionError:
            pass
        # the pattern shows the defect bit for bit: so does the bound
        vr, xr, wr, bound = _random(p)
        worst, _ = ref.worst_ratio(ref.emulate(p, vr, xr, rb, mutant), wr, bound)
        assert worst > 1e6, (mutant, name, worst)
        with pytest.raises(AssertionError):
            ref.assert_rows(ref.emulate(p, vr, xr, rb, mutant), wr, bound,
                            'seeded ' + mutant)
        caught.append((name, what))
    names = set(n for n, _ in caught)
    assert names, mutant
    # ... on the pattern built for it
    expected = {'slack_ignored': 'parity', 'odd_dropped': 'parity',
                'last_pair_dropped': 'full', 'neighbour_added': 'parity',
                'empty_keeps_previous': 'empty_tiles',
                'xcd_remainder_ignored': 'tiles523'}[mutant]
    assert expected in names, (mutant, names)
    if mutant == 'last_pair_dropped':
        assert names == {'full'}
    if mutant == 'empty_keeps_previous':
        assert names <= set(ref.RECT)
        assert ('empty_tiles', 'own') in caught and ('empty_tiles', 'hand') in caught
    if mutant == 'odd_dropped':
        assert 'odd_end_n1' in names and 'odd_end_n333' in names
    if mutant == 'xcd_remainder_ignored':
        assert {'tiles7', 'tiles9', 'tiles523'} <= names
