# -*- coding: utf-8 -*-
'''
Synthetic CSR patterns, two models and a numpy emulation for the fp64
CSR-stream products (helper, not a test): StreamTile / stream_rows_sum /
stream_tile_pair_row_sum of flow_amd/csrc/csr_stream.h and the hand-inlined
copy in spmv_stream_block2_kernel, behind flow_operator_apply (kinds 0, 1, 2,
4), flow_operator_apply_block, the mass residuals (mass_kernels.hip) and the
multigrid level kernels (krylov_kernels.hip).  The fp16 sibling is
tests/fp16_stream_reference.py, whose Pattern, StubLayout, xcd_tile and
comparator are reused here.

Why not meshes: a mesh gives rows of 7-19 entries and regular tiles.  The
patterns here put the tile where it can go wrong -- tiles that start at an odd
nonzero (one slot of alignment slack, ka = k0 - 1), tiles filled to the cap (one
row of `cap` entries, 256 rows), rows of one entry, a trailing odd nonzero whose
pair load reads the padding behind the plane, tile counts around a group of
xcd_tile, and, for the rectangular operators of the multigrid cycle, empty
rows and whole empty tiles at the start, in the middle and at the end.  The
cap is the library's (flow_spmv_tile_nnz), not a number written here.

Two kinds of data, two comparisons:

(1) Exact data: small signed integers, exact zeros among them.  Every product
and every partial sum of a row is an integer below 2^53 (asserted:
`assert_exact`), so the result is the same in any order, with or without
contraction to FMA, and the model is integer arithmetic (numpy.int64).  The
device result of EVERY row must have the model's bit pattern (`assert_bits`):
there is no tolerance to choose.  The multigrid cycle scales by omega * dinv =
2^-1 .. 2^-5: its values are multiples of 2^-5, and 32 times the absolute sum
of every stage stays below 2^53.

(2) Random data (standard_normal): every row against the correctly rounded sum
of the exact products (`exact_row_sums`: Dekker's two-product, math.fsum), with
the bound
    (len + c) 2^-53 sum_k |v_k| |x_k|
derived as in the fp16 helper: the row is an in-order sum of `len` slots from
0.0, a product passes through its own rounding and at most len - 1 additions
(0.0 + slot is exact), and the reference adds its final rounding: c = 1 for
the tiles that park one product per slot.  Kind 2 parks axx u0 + axy u1: a
second product and the slot's addition, one rounding more per product and one
for the reference: c = 3.  To first order, with or without contraction (which
only removes roundings).  A lost or misplaced nonzero moves its row by
~|v| |x|: more than ten orders of magnitude above the bound.
'''
import functools
import math

import numpy

import fp16_stream_reference as ref16
from fp16_stream_reference import (                         # noqa: F401
    Pattern, StubLayout, xcd_tile, assert_rows, blocked, worst_ratio, RATIOS)

U64 = 2.0**-53                  # unit roundoff of fp64
BLOCK = 256                     # kBlock: rows per tile at most
EXACT_MAG = 1 << 10             # |v|, |x| of the square kernels' exact data
MG_MAG = 8                      # |v|, |r| of the multigrid cycle's exact data
MG_GRID = 5                     # the cycle's values are multiples of 2^-5

SQUARE = ('parity', 'full', 'tiles1', 'tiles7', 'tiles9', 'tiles523',
          'odd_end', 'odd_end_n1', 'odd_end_n333')
RECT = ('empty_rows', 'empty_tiles')
# the shapes of the rectangular patterns: on their own (flow_operator_apply)
# and as the operators of a two-level cycle (n = MG_N rows, MG_NC coarse)
MG_N, MG_NC = 1536, 301
RECT_SHAPE = {'empty_rows': (1109, 977), 'empty_tiles': (MG_N, MG_NC)}


def tile_cap(kind=0):
    '''Nonzeros a tile of an operator of `kind` may hold: the library's build
    constant; without a built library the header's.'''
    from flow_amd import _hip
    try:
        return _hip.spmv_tile_nnz(kind)
    except (OSError, _hip.HipError):
        return _hip.SPMV_NNZ_PER_BLOCK


# -- square patterns ----------------------------------------------------------------
def _rows_to(total, nrows):
    '''nrows row lengths that differ by at most one and sum to `total`.'''
    base, rem = divmod(total, nrows)
    assert base >= 1
    return [base + 1] * rem + [base] * (nrows - rem)


def _build_square(name, cap):
    rng = numpy.random.RandomState(2000 + SQUARE.index(name))
    lens, tiles, extra, capped = [], [], {}, []
    if name == 'parity':
        # every tile holds an odd number of nonzeros: k0 alternates even and
        # odd; rows of 1 .. 24 entries
        for t in range(12):
            m = int(rng.randint(8, 40))
            row = [1, 24] + [int(x) for x in rng.choice(
                [1, 1, 2, 3, 5, 8, 13, 21, 24], size=m - 3)]
            row.append(2 if sum(row) % 2 else 1)
            lens += row
            tiles.append(m)
    elif name == 'full':
        # tiles filled to the cap: one row of `cap` entries and 256 rows, each
        # at an even k0 (hi = cap) and at an odd one (hi = cap + 1: the last
        # pair of the tile's LDS slots); 256 rows of one entry
        assert cap % 2 == 0 and cap >= BLOCK + 2

        def rows256():
            # (a row of two entries at least last: its last column is set
            # below)
            rows = [int(x) for x in rng.permutation(_rows_to(cap, BLOCK))]
            k = int(numpy.argmax(rows))
            rows[k], rows[-1] = rows[-1], rows[k]
            return rows

        for part, full in (([cap], True),                       # k0 = 0
                           ([1], False),                        # -> odd
                           ([cap], True),                       # k0 odd
                           (rows256(), True),                   # k0 odd
                           ([1], False),                        # -> even
                           (rows256(), True),                   # k0 even
                           ([1] * BLOCK, False)):
            if full:
                capped.append(len(lens) + len(part) - 1)    # the tile's last row
            lens += [int(x) for x in part]
            tiles.append(len(part))
        ref16._pad_rows(lens, tiles, max(1280, cap + 258), rng)
        # the last nonzero of a capped tile lies off the diagonal: behind it
        for i in capped:
            if lens[i] < cap:
                extra[i] = [i + 1]
    elif name.startswith('tiles'):
        # 523 = one full group of xcd_tile (8 * 64) + a partial one of 11; a
        # few short rows per tile, the last tile fewer
        nt = int(name[5:])
        for t in range(nt):
            m = 9 if t + 1 < nt else 4
            lens += [int(x) for x in rng.choice([1, 1, 2, 3, 4], size=m)]
            tiles.append(m)
    else:
        # an odd number of nonzeros in all: the last pair load reads the entry
        # behind the plane
        n = {'odd_end': 512, 'odd_end_n1': 1, 'odd_end_n333': 333}[name]
        lens = [int(x) for x in rng.choice([1, 2, 3, 4, 5], size=n)]
        if sum(lens) % 2 == 0:
            lens[-1] += 1
        if n == 1:
            lens = [1]
        tiles = [BLOCK] * (n // BLOCK) + ([n % BLOCK] if n % BLOCK else [])
    p = Pattern(name, lens, tiles, rng, extra)
    p.cap = cap
    p.shape = (p.n, p.n)
    # the last nonzero of every capped tile: it carries a definite value
    k0, k1 = p.tile_k()
    p.definite = numpy.array([k - 1 for a, k in zip(k0, k1) if k - a == cap],
                             dtype=numpy.int64)
    check_preconditions(p)
    return p


@functools.lru_cache(maxsize=None)
def square(name, cap):
    return _build_square(name, cap)


# -- rectangular patterns with empty rows ----------------------------------------------
class RectPattern(object):
    '''rowptr, cols (sorted per row, any columns of [0, ncols)), hand-picked
    tiles (rowblocks) over n rows of which some are empty.'''

    def __init__(self, name, shape, lens, tile_rows, rng, cap):
        lens = numpy.asarray(lens, dtype=numpy.int64)
        n, ncols = shape
        assert len(lens) == n and lens.max() <= ncols
        self.name, self.n, self.shape, self.cap = name, n, shape, cap
        self.lens = lens
        self.rowptr = numpy.zeros(n + 1, dtype=numpy.int32)
        numpy.cumsum(lens, out=self.rowptr[1:])
        self.nnz = int(self.rowptr[-1])
        rb = numpy.concatenate([[0], numpy.cumsum(tile_rows)])
        assert rb[-1] == n
        self.rowblocks = rb.astype(numpy.int32)
        cols = numpy.empty(self.nnz, dtype=numpy.int32)
        for i in numpy.nonzero(lens)[0]:
            # (a band around the row's image, as wide as the row needs)
            c = int(i * ncols // n)
            lo = max(0, min(c - 8, ncols - 17))
            pool = numpy.arange(lo, min(ncols, lo + 17))
            if len(pool) < lens[i]:
                pool = numpy.arange(ncols)
            a = self.rowptr[i]
            cols[a:a + lens[i]] = numpy.sort(
                rng.choice(pool, int(lens[i]), replace=False))
        self.cols = cols
        self.row_of = numpy.repeat(numpy.arange(n), lens)
        self.definite = numpy.zeros(0, dtype=numpy.int64)

    def tile_k(self):
        return tile_k(self)

    def own_rowblocks(self):
        '''The product's own partition (multigrid.CsrOperator).'''
        from flow_amd.fem.space import csr_stream_rowblocks
        return csr_stream_rowblocks(self.rowptr, nnz_per_block=self.cap)

    def scipy(self, vals):
        import scipy.sparse as sp
        return sp.csr_matrix((vals, self.cols, self.rowptr), shape=self.shape)


def _build_rect(name, shape, cap, seed):
    rng = numpy.random.RandomState(seed)
    n = shape[0]
    lens, tiles = [], []
    if name == 'empty_rows':
        # empty rows scattered inside tiles, the first and the last row of a
        # tile among them; tiles of many sizes
        sizes = [37, BLOCK, 101, 1, 64, 200, 3, BLOCK, 150]
        t = 0
        while len(lens) < n:
            m = min(sizes[t % len(sizes)], n - len(lens))
            row = [int(x) for x in rng.choice([0, 0, 1, 1, 2, 3, 5], size=m)]
            if t % 3 != 2 or m == 1:
                row[0] = 0
                row[-1] = 0
            if m > 2:
                row[1] = 2          # (the tile of ONE row may be empty)
            lens += row
            tiles.append(m)
            t += 1
    else:
        # whole tiles of 256 empty rows: the first (k0 = k1 = 0), one in the
        # middle at an odd k0, the last (k0 = k1 = nnz, odd)
        assert n == 6 * BLOCK
        for m in (0, 100, 156, 0, 77, 179, BLOCK, 0):
            if m == 0:
                if sum(lens) % 2 == 0 and lens:
                    lens[-1] += 1                # -> an odd k0 = k1
                lens += [0] * BLOCK
                tiles.append(BLOCK)
                continue
            row = [int(x) for x in rng.choice([0, 1, 1, 2, 3], size=m)]
            row[-1] = max(row[-1], 1)
            lens += row
            tiles.append(m)
    p = RectPattern(name, shape, lens, tiles, rng, cap)
    check_preconditions(p)
    return p


@functools.lru_cache(maxsize=None)
def rect(name, cap, shape=None):
    shape = shape or RECT_SHAPE[name]
    return _build_rect(name, shape, cap, 3000 + RECT.index(name) + 7 * shape[0]
                       + shape[1])


def pattern(name, cap):
    return square(name, cap) if name in SQUARE else rect(name, cap)


def tile_k(p, rowblocks=None):
    '''(k0, k1): the first nonzero and the end of every tile.'''
    rb = numpy.asarray(p.rowblocks if rowblocks is None else rowblocks,
                       dtype=numpy.int64)
    rp = p.rowptr.astype(numpy.int64)
    return rp[rb[:-1]], rp[rb[1:]]


def tile_parities(p, rowblocks=None):
    '''k0 % 2 of the tiles that hold nonzeros.'''
    k0, k1 = tile_k(p, rowblocks)
    return set(int(x) for x in (k0 % 2)[k1 > k0])


def tile_hi(p, rowblocks=None):
    '''k1 - (k0 aligned down to even) per tile: `hi` of the tile routine, at
    most cap + 1 = kTile - 1.'''
    k0, k1 = tile_k(p, rowblocks)
    return k1 - (k0 & ~1)


def empty_tiles(p, rowblocks=None):
    '''Indices of the tiles without a nonzero.'''
    k0, k1 = tile_k(p, rowblocks)
    return numpy.nonzero(k1 == k0)[0]


def check_preconditions(p, rowblocks=None):
    '''What the kernels rely on (nothing in them checks it) -- a valid CSR
    pattern with sorted columns in range, tiles of at most 256 rows and `cap`
    nonzeros that cover all rows in order -- and that the edge a pattern is
    named after is really there.'''
    rb = numpy.asarray(p.rowblocks if rowblocks is None else rowblocks,
                       dtype=numpy.int64)
    rp = p.rowptr.astype(numpy.int64)
    n, ncols = p.shape
    assert rp[0] == 0 and (numpy.diff(rp) >= 0).all() and rp[-1] == len(p.cols)
    assert p.nnz > 0 and p.cols.min() >= 0 and p.cols.max() < ncols
    assert (numpy.diff(p.cols) > 0)[numpy.diff(p.row_of) == 0].all()
    assert rb[0] == 0 and rb[-1] == n and (numpy.diff(rb) >= 1).all()
    assert numpy.diff(rb).max() <= BLOCK
    assert numpy.diff(rp[rb]).max() <= p.cap
    hi = tile_hi(p, rb)
    assert hi.max() <= p.cap + 1
    name = p.name
    if name in SQUARE:
        assert (numpy.diff(rp) >= 1).all()
        assert (p.cols[p.diag_idx] == numpy.arange(n)).all()
    if name in ('parity', 'full', 'tiles523'):
        assert tile_parities(p, rb) == {0, 1}
    if name == 'parity':
        k0, k1 = tile_k(p, rb)
        assert ((k1 - k0) % 2 == 1).all() and len(k0) >= 12
        assert p.lens.min() == 1 and p.lens.max() == 24
    if name == 'full':
        k0, k1 = tile_k(p, rb)
        rows = numpy.diff(rb)
        full = (k1 - k0) == p.cap
        for nrows in (1, BLOCK):
            assert set(k0[full & (rows == nrows)] % 2) == {0, 1}, nrows
        assert (hi == p.cap + 1).sum() == 2
        assert ((rows == BLOCK) & (k1 - k0 == BLOCK)).any()
        assert len(p.definite) == 4
        assert (p.cols[p.definite] != p.row_of[p.definite]).all()
    if name.startswith('tiles'):
        rows = numpy.diff(rb)
        assert len(rows) == int(name[5:]) and n < 5000
        assert len(rows) == 1 or rows[-1] < rows[0]
    if name.startswith('odd_end'):
        assert p.nnz % 2 == 1
        assert n == {'odd_end': 512, 'odd_end_n1': 1, 'odd_end_n333': 333}[name]
    if name == 'empty_rows':
        lens = numpy.diff(rp)
        assert 0.1 * n < (lens == 0).sum() < 0.6 * n
        assert tile_parities(p, rb) == {0, 1}
        if rowblocks is None:       # (the hand-picked tiles)
            assert (lens[rb[:-1]] == 0).any() and (lens[rb[1:] - 1] == 0).any()
            assert (lens[rb[:-1]] > 0).any() and (lens[rb[1:] - 1] > 0).any()
    if name == 'empty_tiles':
        k0, k1 = tile_k(p, rb)
        e = empty_tiles(p, rb)
        assert e[0] == 0 and e[-1] == len(rb) - 2 and len(e) >= 3
        assert k0[e[-1]] == p.nnz and p.nnz % 2 == 1
        assert (k0[e[1:-1]] % 2 == 1).any()
        assert (numpy.diff(rb)[e] == BLOCK).all()


# -- data ---------------------------------------------------------------------------------
def _definite_columns(p):
    return p.cols[p.definite]


def exact_data(p, seed, planes=4, mag=EXACT_MAG, ncomp=2):
    '''(values (planes, nnz), vector (ncomp * ncols)) as int64: signed
    integers up to `mag` in absolute value, a tenth of them zero, a nonzero
    diagonal where the pattern has one, the last nonzero of a capped tile and
    the vector at its column definite.'''
    rng = numpy.random.RandomState(seed)
    ncols = p.shape[1]
    v = rng.randint(-mag, mag + 1, size=(planes, p.nnz)).astype(numpy.int64)
    v[rng.uniform(size=v.shape) < 0.1] = 0
    v[:, ::97] = mag
    v[:, 5::89] = -mag
    if hasattr(p, 'diag_idx'):
        d = v[:, p.diag_idx]
        v[:, p.diag_idx] = numpy.where(d == 0, 3, d)
    v[:, p.definite] = -(mag - 1)
    x = rng.randint(-mag, mag + 1, size=ncomp * ncols).astype(numpy.int64)
    x[rng.uniform(size=x.shape) < 0.1] = 0
    x[::53] = mag
    x[7::59] = -mag
    for c in range(ncomp):
        x[c * ncols + _definite_columns(p)] = mag - 2 - c
    return v, x


def random_data(p, seed, planes=4, ncomp=2):
    '''The same shapes from standard_normal (float64); the definite entries
    O(1).'''
    rng = numpy.random.RandomState(seed)
    ncols = p.shape[1]
    v = rng.standard_normal((planes, p.nnz))
    x = rng.standard_normal(ncomp * ncols)
    v[:, p.definite] = -0.75
    for c in range(ncomp):
        x[c * ncols + _definite_columns(p)] = 1.5 + c
    return v, x


def row_mask(p, seed=77):
    '''Row mask of kind 4 (2n, component-blocked): about 15 % identity rows
    (0).'''
    rng = numpy.random.RandomState(seed)
    return (rng.uniform(size=2 * p.n) > 0.15).astype(numpy.uint8)


# -- the models ------------------------------------------------------------------------------
def row_terms(kind, p, planes, x):
    '''Per component of the result, the (values, gathered vector) pairs whose
    products a row sums: kind 0 one plane; 1 a plane per component; 2 the 2x2
    blocks (plane 2 r + s: test component r, trial component s); 4 one plane
    for both components.'''
    ncols = p.shape[1]
    g = [x[c * ncols + p.cols] for c in range(len(x) // ncols)]
    if kind == 0:
        return [[(planes[0], g[0])]]
    if kind == 1:
        return [[(planes[0], g[0])], [(planes[1], g[1])]]
    if kind == 2:
        return [[(planes[0], g[0]), (planes[1], g[1])],
                [(planes[2], g[0]), (planes[3], g[1])]]
    assert kind == 4
    return [[(planes[0], g[0])], [(planes[0], g[1])]]


def _row_add(p, t):
    out = numpy.zeros(p.n, dtype=t.dtype)
    numpy.add.at(out, p.row_of, t)
    return out


def int_product(kind, p, planes, x, mask=None):
    '''The integer model: (result (ncomp * n) as int64, per row the sum of the
    absolute values of its terms).  mask (kind 4): 0 = the row returns x.'''
    assert planes.dtype == numpy.int64 and x.dtype == numpy.int64
    out, sabs = [], []
    for c, terms in enumerate(row_terms(kind, p, planes, x)):
        s = sum(_row_add(p, v * g) for v, g in terms)
        a = sum(_row_add(p, numpy.abs(v * g)) for v, g in terms)
        if mask is not None:
            own = x[c * p.n:(c + 1) * p.n]
            ident = mask[c * p.n:(c + 1) * p.n] == 0
            s, a = numpy.where(ident, own, s), numpy.where(ident, abs(own), a)
        out.append(s)
        sabs.append(a)
    return numpy.concatenate(out), numpy.concatenate(sabs)


def assert_exact(sabs, what, grid=0):
    '''The condition under which "exact" holds: 2^grid times the absolute sum
    of every row's terms is an integer below 2^53.'''
    top = int(numpy.max(sabs)) << grid
    assert top < 2**53, '%s: sum of |terms| = %d * 2^-%d' % (what, top, grid)
    return top


def _two_prod(a, b):
    '''p + e == a * b exactly (Dekker / Veltkamp; no overflow at these
    magnitudes).'''
    p = a * b
    ca, cb = 134217729.0 * a, 134217729.0 * b
    ah = ca - (ca - a)
    bh = cb - (cb - b)
    al, bl = a - ah, b - bh
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    return p, e


def exact_row_sums(p, terms):
    '''The correctly rounded row sums of the EXACT products of `terms`
    [(values, gathered vector)], and per row sum |v| |x|.'''
    parts = []
    sabs = numpy.zeros(p.n)
    for v, g in terms:
        parts += list(_two_prod(v, g))
        sabs += _row_add(p, numpy.abs(v * g))
    rp = p.rowptr
    s = numpy.array([math.fsum(numpy.concatenate([q[rp[i]:rp[i + 1]]
                                                  for q in parts]))
                     for i in range(p.n)]) if p.n else numpy.zeros(0)
    return s, sabs


def float_product(kind, p, planes, x, mask=None):
    '''The random-data model: (result (ncomp * n), bound per row) with the
    bound of the module docstring; identity rows (mask 0) return x and ask
    for equality.'''
    c_extra = 3.0 if kind == 2 else 1.0
    out, bound = [], []
    for c, terms in enumerate(row_terms(kind, p, planes, x)):
        s, sabs = exact_row_sums(p, terms)
        b = (p.lens + c_extra) * U64 * sabs
        if mask is not None:
            ident = mask[c * p.n:(c + 1) * p.n] == 0
            s = numpy.where(ident, x[c * p.n:(c + 1) * p.n], s)
            b = numpy.where(ident, 0.0, b)
        out.append(s)
        bound.append(b)
    return numpy.concatenate(out), numpy.concatenate(bound)


def bits(a):
    a = numpy.ascontiguousarray(a)
    return a.view({4: numpy.uint32, 8: numpy.uint64}[a.dtype.itemsize])


def assert_bits(got, want, what):
    '''Every entry of `got` has the bit pattern of the model (`want`: int64,
    or floats of got's type).'''
    got = numpy.asarray(got)
    want = numpy.asarray(want)
    if want.dtype.kind == 'i':
        assert numpy.abs(want).max(initial=0) < 2**53
    want = want.astype(got.dtype)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = numpy.nonzero(bits(got) != bits(want))
    assert len(bad[0]) == 0, (
        '%s: %d of %d entries differ from the exact model, the first at %s '
        '(got %r, expected %r)' % (what, len(bad[0]), got.size,
                                   tuple(b[0] for b in bad),
                                   got[tuple(b[0] for b in bad)],
                                   want[tuple(b[0] for b in bad)]))


# -- the multigrid cycle ------------------------------------------------------------------
def mg_operators(cap, seed=91):
    '''The rectangular patterns as a two-level hierarchy with integer entries
    (|v| <= MG_MAG): dict of Ah (n x n, empty rows), Ps (n x nc, empty rows and
    empty tiles), R (nc x n), each a (pattern, int64 values) pair, the exponents
    e of dinv = 2^-e (0 .. 4) and the residual r (int64).'''
    rng = numpy.random.RandomState(seed)
    pats = dict(Ah=rect('empty_rows', cap, (MG_N, MG_N)),
                Ps=rect('empty_tiles', cap, (MG_N, MG_NC)),
                R=rect('empty_rows', cap, (MG_NC, MG_N)))
    ops = {}
    for i, (key, p) in enumerate(sorted(pats.items())):
        v, _ = exact_data(p, seed + i, planes=1, mag=MG_MAG, ncomp=1)
        ops[key] = (p, v[0])
    ops['dinv_exp'] = rng.randint(0, 5, size=MG_N).astype(numpy.int64)
    r = rng.randint(-MG_MAG, MG_MAG + 1, size=MG_N).astype(numpy.int64)
    r[rng.uniform(size=MG_N) < 0.1] = 0
    ops['r'] = r
    return ops


def mg_restriction(ops):
    '''C = R - R Ah, formed exactly in integers (scipy CSR, zeros removed).'''
    Ah, R = [ops[k][0].scipy(ops[k][1]) for k in ('Ah', 'R')]
    C = (R - R.dot(Ah)).tocsr().astype(numpy.int64)
    C.eliminate_zeros()
    C.sort_indices()
    return C


def mg_model(ops, fused, coarse_identity=True):
    '''One cycle of flow_mg_apply with Ainv the identity (or zero), omega =
    1/2, in integers: dict of t = r - Ah r (non-fused form only), r1 (= R t,
    or C r), x1, z32 = 32 z -- and `sabs`: per stage 32 times the absolute sum
    of the row's terms, for assert_exact.
      non-fused  z = Ps x1 + omega dinv (r + t)
      fused      z = Ps x1 + omega dinv (2 r - Ah r)
    (r + t and 2 r - Ah r are the same integer; omega dinv = 2^-(e + 1))'''
    (pa, va), (pp, vp), (pr, vr) = ops['Ah'], ops['Ps'], ops['R']
    r, e = ops['r'], ops['dinv_exp']
    Ar, Ar_abs = int_product(0, pa, va[None], r)
    t = r - Ar
    out = {'t': t}
    sabs = {'t': 32 * (numpy.abs(r) + Ar_abs)}
    if fused:
        C = mg_restriction(ops)
        r1 = C.dot(r)
        sabs['r1'] = 32 * abs(C).dot(numpy.abs(r))
        assert numpy.array_equal(r1, int_product(0, pr, vr[None], t)[0])
    else:
        r1, r1_abs = int_product(0, pr, vr[None], t)
        sabs['r1'] = 32 * r1_abs
    x1 = r1 if coarse_identity else numpy.zeros_like(r1)
    Px, Px_abs = int_product(0, pp, vp[None], x1)
    w = numpy.left_shift(1, 4 - e)                  # 32 omega dinv
    out.update(r1=r1, x1=x1, z32=32 * Px + w * (r + t))
    # (the fused epilogue forms 2 r - Ah r from its terms)
    sabs['z'] = 32 * Px_abs + w * ((2 if fused else 1) * numpy.abs(r) + (
        Ar_abs if fused else numpy.abs(t)))
    out['sabs'] = sabs
    return out


# -- the tile as the header states it, in numpy ----------------------------------------------
MUTANTS = ('slack_ignored', 'odd_dropped', 'last_pair_dropped',
           'neighbour_added', 'empty_keeps_previous', 'xcd_remainder_ignored')


def xcd_tile_remainder_ignored(b, nwg):
    '''xcd_tile with the partial group's runs all of q tiles (its r longer
    runs forgotten): not a bijection when r > 0.  (The identity in place of
    the partial group's mapping IS a bijection: every tile is still done once,
    and no comparison of results can or need see it.)'''
    group = 8 * ref16.XCD_RUN
    full = (nwg // group) * group
    if b < full:
        return xcd_tile(b, nwg)
    nt, i = nwg - full, b - full
    return full + (i & 7) * (nt >> 3) + (i >> 3)


def emulate(p, vals, x, rowblocks=None, mutant=None):
    '''y = A x through the tile of csr_stream.h (StreamTile), workgroup by
    workgroup: ka = k0 & ~1, pair loads up to npair = (k1 - ka + 1) >> 1 from
    arrays padded as the product pads them, x gathered for [k0, k1) only (the
    tile's first column elsewhere), the products parked in kTile = cap + 2 LDS
    slots, the in-order sum of [a, b) per lane.  Rows no workgroup writes stay
    NaN.  mutant: one seeded defect (MUTANTS).'''
    assert mutant is None or mutant in MUTANTS
    rb = numpy.asarray(p.rowblocks if rowblocks is None else rowblocks,
                       dtype=numpy.int64)
    rp = p.rowptr.astype(numpy.int64)
    ktile = p.cap + 2
    pad = 2 + (p.nnz & 1)
    cols = numpy.concatenate([p.cols.astype(numpy.int64),
                              numpy.zeros(pad, dtype=numpy.int64)])
    v = numpy.concatenate([numpy.asarray(vals, dtype=numpy.float64),
                           numpy.zeros(pad)])
    x = numpy.asarray(x, dtype=numpy.float64)
    nt = len(rb) - 1
    y = numpy.full(p.n, numpy.nan)
    mapping = xcd_tile_remainder_ignored if mutant == 'xcd_remainder_ignored' \
        else xcd_tile
    previous = numpy.zeros(BLOCK)
    for wg in range(nt):
        tile = mapping(wg, nt)
        if not 0 <= tile < nt:
            continue
        r0, r1 = rb[tile], rb[tile + 1]
        k0, k1 = rp[r0], rp[r1]
        ka = k0 & ~1
        a = numpy.zeros(BLOCK, dtype=numpy.int64)
        b = numpy.zeros(BLOCK, dtype=numpy.int64)
        base = k0 if mutant == 'slack_ignored' else ka
        a[:r1 - r0] = rp[r0:r1] - base
        b[:r1 - r0] = rp[r0 + 1:r1 + 1] - base
        npair = (k1 - ka + 1) >> 1
        if mutant == 'odd_dropped':
            npair = (k1 - ka) >> 1
        if mutant == 'last_pair_dropped':
            npair = min(npair, p.cap // 2)
        assert 2 * npair <= ktile and ka + 2 * npair <= len(v)
        prod = numpy.full(ktile, numpy.nan)           # (LDS starts undefined)
        s = numpy.zeros(BLOCK)
        if k0 < k1:
            lo, hi = k0 - ka, k1 - ka
            safe = cols[k0]
            e = 2 * numpy.arange(npair)
            c0, c1 = cols[ka + e], cols[ka + e + 1]
            own1 = e + 1 < hi
            if mutant == 'neighbour_added' and k1 < p.nnz:
                own1 = e + 1 < hi + 1
                if r1 > r0:
                    b[r1 - r0 - 1] += (hi & 1)
            g0 = x[numpy.where((e >= lo) & (e < hi), c0, safe)]
            g1 = x[numpy.where(own1, c1, safe)]
            prod[e] = v[ka + e] * g0
            prod[e + 1] = v[ka + e + 1] * g1
            for j in range(int((b - a).max())):
                rows = numpy.nonzero(b - a > j)[0]
                s[rows] = s[rows] + prod[a[rows] + j]
        elif mutant == 'empty_keeps_previous':
            s = previous
        y[r0:r1] = s[:r1 - r0]
        previous = s
    return y
