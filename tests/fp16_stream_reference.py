# -*- coding: utf-8 -*-
'''
Synthetic CSR patterns, an exact model and the comparator for the fp16
CSR-stream products (helper, not a test): fp16_tile_row_sum of
flow_amd/csrc/csr_stream16.h behind the mass solver's plain and packed streams
(mass_kernels.hip) and the three p-multigrid level formats (pmg_kernels.hip).

Why not meshes: a mesh gives rows of 7-19 entries and regular tiles.  The
patterns here put the tile routine where it can go wrong -- a tile that starts
at every residue of the quad alignment, tiles filled to the cap of 2044
nonzeros (one row of 2044, 256 rows), rows of one entry, tile counts around a
group of xcd_tile, column spans of exactly 65535 (16-bit offsets fit) and 65536
(they do not).  The tests pick the tiles (`rowblocks`) themselves: the kernels
take any partition with at most 256 rows and 2044 nonzeros per tile.

The model (`tile_product`) is float64 arithmetic on the fp16-rounded weights
widened exactly; the rounding of the setup kernels (double -> half of
v * (1 / d), once), the tiles' base columns, 16-bit offsets, packed words, identity
rows and the Chebyshev coefficients are restated next to it.

The bound of the comparison is derived, not tuned.  A row's sum is an in-order
fp32 sum of `len` products: every product passes through at most `len`
roundings (its own and the additions behind it), the epilogue adds at most four
more (a scaling, a subtraction, an axpy).  With u = 2^-24 the error of the row
is at most
    (len + 4) u (sum_k |w_k| |g_k| + |epilogue operands|)
to first order, with or without contraction to FMA (which only removes
roundings).  A lost or misplaced nonzero moves its row by ~|w| |g|: four orders
of magnitude more.
'''
import functools

import numpy

U32 = 2.0**-24                  # unit roundoff of fp32
BLOCK = 256                     # kBlock: rows per tile at most
TILE_NNZ = 2044                 # kTile16 - 4: nonzeros per tile at most
XCD_RUN = 64                    # kXcdRun (common.h)

PATTERNS = ('residues', 'full', 'tiles1', 'tiles7', 'tiles9', 'tiles523',
            'wide', 'wide_overflow')
WIDE_N = 65600
WIDE_TILE = 1                   # the tile that carries the span
WIDE_CMIN = 17


# -- patterns -------------------------------------------------------------------
class Pattern(object):
    '''rowptr, cols (sorted per row, the diagonal in every row), diag_idx, the
    tiles (rowblocks) and fp64 values: `vals` (the mass solver's one plane),
    `a00` / `a11` (the two diagonal blocks of a p-multigrid level) and
    `rowmask` (2n; 0 = identity row of the pair mass operator).'''

    def __init__(self, name, lens, tile_rows, rng, extra=None):
        lens = numpy.asarray(lens, dtype=numpy.int64)
        n = len(lens)
        self.name, self.n = name, n
        self.rowptr = numpy.zeros(n + 1, dtype=numpy.int32)
        numpy.cumsum(lens, out=self.rowptr[1:])
        self.nnz = int(self.rowptr[-1])
        rb = numpy.concatenate([[0], numpy.cumsum(tile_rows)])
        assert rb[-1] == n
        self.rowblocks = rb.astype(numpy.int32)
        cols = numpy.empty(self.nnz, dtype=numpy.int32)
        extra = extra or {}
        for i in range(n):
            a, L = self.rowptr[i], int(lens[i])
            if L == 1:
                cols[a] = i
                continue
            fixed = numpy.asarray(extra.get(i, []), dtype=numpy.int64)
            # the other columns: near the diagonal, as far as the row needs
            half = max(8, L)
            lo, hi = max(0, i - half), min(n, i + half + 1)
            if hi - lo < L:
                lo, hi = 0, n
            pool = numpy.setdiff1d(numpy.arange(lo, hi),
                                   numpy.concatenate([[i], fixed]))
            pick = rng.choice(pool, L - 1 - len(fixed), replace=False)
            cols[a:a + L] = numpy.sort(numpy.concatenate([[i], fixed, pick]))
        self.cols = cols
        self.row_of = numpy.repeat(numpy.arange(n), lens)
        self.diag_idx = numpy.nonzero(cols == self.row_of)[0].astype(numpy.int32)
        assert len(self.diag_idx) == n
        self.lens = lens
        # (one sign per row for all planes: the one-plane level divides by the
        # MEAN of the two blocks' diagonals)
        self.sign = numpy.where(rng.uniform(size=n) < 0.2, -1.0, 1.0)
        self.vals = self._values(rng)
        self.a00 = self._values(rng)
        self.a11 = self._values(rng)
        # rows whose off-diagonal entries vanish in block 0 only, in block 1
        # only, in both: identity rows of pmg_pack1_kernel (rows of one entry
        # are identity rows of both blocks anyway)
        long_rows = numpy.nonzero(lens > 1)[0]
        pick = rng.permutation(long_rows)[:max(3, len(long_rows) // 6)]
        off = numpy.ones(self.nnz, dtype=bool)
        off[self.diag_idx] = False
        for j, planes in enumerate(([self.a00], [self.a11],
                                    [self.a00, self.a11])):
            rows = numpy.zeros(n, dtype=bool)
            rows[pick[j::3]] = True
            for plane in planes:
                plane[off & rows[self.row_of]] = 0.0
        self.rowmask = (rng.uniform(size=2 * n) > 0.15).astype(numpy.uint8)

    def _values(self, rng):
        '''Random signed entries; the diagonal (0.5 .. 4, either sign) is such
        that the scaled entries v / d are log-uniform over the fp16 normal
        range -- up to 1 in short rows, up to 16 / len in long ones, so that
        the absolute row sums stay O(1) as in a Jacobi-scaled matrix --, with
        some fp16 subnormals (|v / d| < 6.1e-5) and exact zeros among them.'''
        n, nnz, L = self.n, self.nnz, self.lens[self.row_of]
        d = rng.uniform(0.5, 4.0, size=n) * self.sign
        top = numpy.log2(numpy.minimum(1.0, 16.0 / L))
        t = 2.0**(-14.0 + rng.uniform(size=nnz) * (14.0 + top))
        kind = rng.uniform(size=nnz)
        t = numpy.where(kind < 0.12, 2.0**(-15.0 - 9.0 * rng.uniform(size=nnz)), t)
        t = numpy.where(kind < 0.06, 0.0, t)
        t *= numpy.where(rng.uniform(size=nnz) < 0.5, -1.0, 1.0)
        v = t * d[self.row_of]
        v[self.diag_idx] = d
        return v

    # what the tests assert to occur ------------------------------------------
    def tile_k(self):
        rp = self.rowptr.astype(numpy.int64)
        return rp[self.rowblocks[:-1]], rp[self.rowblocks[1:]]

    def residues(self):
        k0, _k1 = self.tile_k()
        return set(int(r) for r in k0 % 4)

    def tile_hi(self):
        '''k1 - (k0 aligned down to a multiple of four) per tile: `hi` of
        fp16_tile_row_sum, at most kTile16 - 1 = 2047.'''
        k0, k1 = self.tile_k()
        return k1 - (k0 & ~3)

    def tile_spans(self):
        k0, k1 = self.tile_k()
        c = self.cols.astype(numpy.int64)
        return numpy.array([c[a:b].max() - c[a:b].min()
                            for a, b in zip(k0, k1)])


def _pad_rows(lens, tiles, n, rng):
    '''Short rows in tiles of 64 up to n rows (a row of 2044 entries needs as
    many columns).'''
    while len(lens) < n:
        m = min(64, n - len(lens))
        lens += [int(x) for x in rng.randint(1, 6, size=m)]
        tiles.append(m)


def _build(name):
    rng = numpy.random.RandomState(
        1000 + PATTERNS.index(name))
    lens, tiles, extra = [], [], None
    if name == 'residues':
        # every tile holds 1 (mod 4) nonzeros: the first nonzeros of the tiles
        # run through k0 % 4 = 0, 1, 2, 3, 0, ...; rows of 1 .. 24 entries
        for t in range(13):
            m = int(rng.randint(8, 40))
            row = [1] + [int(x) for x in rng.choice(
                [1, 1, 2, 3, 5, 8, 13, 21], size=m - 1)]
            row[-1] += (1 - sum(row)) % 4
            lens += row
            tiles.append(m)
    elif name == 'full':
        # tiles filled to the cap of 2044 nonzeros, at k0 % 4 == 0 (hi = 2044)
        # and at k0 % 4 == 3 (hi = 2047, the last product slot of the tile)
        rows256 = [8] * 252 + [7] * 4
        assert sum(rows256) == TILE_NNZ
        for part, m in (([TILE_NNZ], 1),          # k0 = 0
                        ([1, 2], 2),              # k0 = 2044 -> 2047
                        (list(rng.permutation(rows256)), 256),   # k0 % 4 == 3
                        ([TILE_NNZ], 1),          # k0 % 4 == 3
                        ([1], 1),                 # -> k0 % 4 == 0
                        (list(rng.permutation(rows256)), 256),   # k0 % 4 == 0
                        ([1] * 256, 256)):
            lens += [int(x) for x in part]
            tiles.append(m)
        _pad_rows(lens, tiles, 2304, rng)
    elif name.startswith('tiles'):
        # 523 = one full group of xcd_tile (8 * 64) + a partial one of 11 (runs
        # of 2 and 1); a few short rows per tile, the last tile fewer
        nt = int(name[5:])
        for t in range(nt):
            m = 9 if t + 1 < nt else 4
            lens += [int(x) for x in rng.choice([1, 1, 2, 3, 4], size=m)]
            tiles.append(m)
    else:
        # 65600 rows, mostly of one entry; tile WIDE_TILE holds the columns
        # WIDE_CMIN and WIDE_CMIN + 65535 (+ 1: the offsets overflow 16 bits)
        n = WIDE_N
        lens = numpy.ones(n, dtype=numpy.int64)
        some = numpy.concatenate([numpy.arange(3, n, 16), numpy.arange(4, n, 16),
                                  numpy.arange(6, n, 16)])
        lens[some] = rng.randint(2, 6, size=len(some))
        tiles = [BLOCK] * (n // BLOCK) + [n % BLOCK]
        r0 = WIDE_TILE * BLOCK
        span = 65535 if name == 'wide' else 65536
        lens[r0 + 5], lens[r0 + 200] = 3, 4
        lens[WIDE_CMIN], lens[WIDE_CMIN + span] = 3, 3
        extra = {r0 + 5: [WIDE_CMIN], r0 + 200: [WIDE_CMIN + span]}
    p = Pattern(name, lens, tiles, rng, extra)
    for row, fixed in (extra or {}).items():
        # the two entries that make the span carry a definite weight in every
        # format (the one-plane level drops entries whose row or column is an
        # identity row: neither is)
        for i, j in ((row, fixed[0]), (fixed[0], None)):
            a, b = p.rowptr[i], p.rowptr[i + 1]
            k = a + (int(numpy.searchsorted(p.cols[a:b], j)) if j is not None
                     else int(p.cols[a] == i))
            assert k != p.diag_idx[i] and (j is None or p.cols[k] == j)
            for plane in (p.vals, p.a00, p.a11):
                plane[k] = 0.375 * plane[p.diag_idx[i]]
    if name == 'full':
        # the last nonzero of the 256-row tiles filled to the cap (the product
        # slots 2046 and 2043 of the tile) carries a definite weight
        k0, k1 = p.tile_k()
        for k in k1[(k1 - k0 == TILE_NNZ) & (numpy.diff(p.rowblocks) == BLOCK)] - 1:
            i = p.row_of[k]
            if k != p.diag_idx[i]:
                for plane in (p.vals, p.a00, p.a11):
                    plane[k] = 0.375 * plane[p.diag_idx[i]]
    check_preconditions(p)
    return p


@functools.lru_cache(maxsize=None)
def pattern(name):
    return _build(name)


def check_preconditions(p):
    '''What the kernels rely on (nothing in them checks it): a valid CSR
    pattern with columns in [0, n), tiles of at most 256 rows and 2044
    nonzeros that cover all rows in order.'''
    rp, rb = p.rowptr.astype(numpy.int64), p.rowblocks.astype(numpy.int64)
    assert rp[0] == 0 and (numpy.diff(rp) >= 1).all() and rp[-1] == len(p.cols)
    assert p.cols.min() >= 0 and p.cols.max() < p.n
    for i in (0, p.n // 2, p.n - 1):
        c = p.cols[rp[i]:rp[i + 1]]
        assert (numpy.diff(c) > 0).all()
    assert (numpy.diff(p.cols) > 0)[numpy.diff(p.row_of) == 0].all()
    assert (p.cols[p.diag_idx] == numpy.arange(p.n)).all()
    assert rb[0] == 0 and rb[-1] == p.n and (numpy.diff(rb) >= 1).all()
    assert numpy.diff(rb).max() <= BLOCK
    assert numpy.diff(rp[rb]).max() <= TILE_NNZ
    assert p.tile_hi().max() <= 4 * 2 * BLOCK - 1


class StubLayout(object):
    '''What fmass.MassSolver, pmg._Level and ops.Matrix ask of a layout, over a
    Pattern: N, nnz, degree, pattern(), dev(), _dev -- with the tiles of the
    test pre-seeded as the fp16 kernels' row blocks.  The device copies are
    made by the product's own ScalarLayout.dev (its padding of `cols`).'''
    degree = 1

    def __init__(self, p):
        from flow_amd import device
        self.N, self.nnz = p.n, p.nnz
        # (rowblocks / rowblocks2 belong to the fp64 products of ops.Matrix,
        # which these tests never launch: their tile is smaller than 2044)
        self._pattern = {'rowptr': p.rowptr, 'cols': p.cols, 'nnz': p.nnz,
                         'diag_idx': p.diag_idx, 'rowblocks': p.rowblocks,
                         'rowblocks2': p.rowblocks}
        self._dev = {'pmg_rowblocks': device.to_device(p.rowblocks)}

    def pattern(self, name):
        return self._pattern[name]

    def dev(self, name):
        from flow_amd.fem.space import ScalarLayout
        return ScalarLayout.dev(self, name)


# -- what the setup kernels write ---------------------------------------------
def round16(v, d):
    '''half(v * (1 / d)): mass_pack_kernel, mass_pack16_kernel,
    pmg_pack_kernel, pmg_pack1_kernel (half_rn of csr_stream16.h) -- the
    reciprocal first, then a multiply, and ONE rounding to nearest even from
    the fp64 product.  Through float (two roundings) the result is one fp16
    ulp off wherever the product lies within half a float ulp of a tie of the
    fp16 grid: 2^-13 of all entries (round16_via_float; the GPU tests found
    the kernels, written with the float in between, compiled to the single
    rounding).'''
    inv = 1.0 / numpy.asarray(d, dtype=numpy.float64)
    with numpy.errstate(under='ignore'):
        return (numpy.asarray(v, dtype=numpy.float64) * inv).astype(numpy.float16)


def round16_via_float(v, d):
    '''double -> float -> half: what round16 is NOT.'''
    inv = 1.0 / numpy.asarray(d, dtype=numpy.float64)
    with numpy.errstate(under='ignore'):
        return numpy.float32(numpy.asarray(v, dtype=numpy.float64) * inv).astype(
            numpy.float16)


def mass_weights(p):
    '''vals16 of flow_mass.'''
    return round16(p.vals, p.vals[p.diag_idx][p.row_of])


def pmg_two_planes(p):
    '''pmg_pack_kernel: (vals as (nnz, 2) halves, diag, dinv as (n, 2)
    floats).'''
    w, diag, dinv = [], [], []
    for a in (p.a00, p.a11):
        d = a[p.diag_idx]
        w.append(round16(a, d[p.row_of]))
        diag.append(numpy.float32(d))
        dinv.append(numpy.float32(1.0 / d))
    return (numpy.stack(w, axis=1), numpy.stack(diag, axis=1),
            numpy.stack(dinv, axis=1))


def pmg_idrows(p):
    '''pmg_idrows_kernel: (n, 2) flags, 1 = no nonzero off-diagonal entry in
    that block.'''
    off = numpy.ones(p.nnz, dtype=bool)
    off[p.diag_idx] = False
    out = []
    for a in (p.a00, p.a11):
        cnt = numpy.bincount(p.row_of, weights=(off & (a != 0.0)).astype(float), minlength=p.n)
        out.append((cnt == 0).astype(numpy.uint8))
    return numpy.stack(out, axis=1)


def pmg_one_plane(p):
    '''pmg_pack1_kernel: (weights as halves, idrows (n, 2), diag, dinv (n, 2)).
    Entry (i, j): the mean over the components in which neither row i nor
    column j is an identity row, over the mean diagonal of row i's free
    components; identity rows keep their blocks' own diag / dinv.'''
    idr = pmg_idrows(p)
    f0, f1 = idr[:, 0] == 0, idr[:, 1] == 0
    e0, e1 = p.a00[p.diag_idx], p.a11[p.diag_idx]
    d = numpy.where(f0 & f1, 0.5 * (e0 + e1),
                    numpy.where(f0, e0, numpy.where(f1, e1, 1.0)))
    d0, d1 = numpy.where(f0, d, e0), numpy.where(f1, d, e1)
    diag = numpy.stack([numpy.float32(d0), numpy.float32(d1)], axis=1)
    dinv = numpy.stack([numpy.float32(1.0 / d0), numpy.float32(1.0 / d1)], axis=1)
    i, j = p.row_of, p.cols
    u0, u1 = f0[i] & f0[j], f1[i] & f1[j]
    v = numpy.where(u0 & u1, 0.5 * (p.a00 + p.a11),
                    numpy.where(u0, p.a00, numpy.where(u1, p.a11, 0.0)))
    return round16(v, d[i]), idr, diag, dinv


def tile_bases(p):
    '''tile_lowest_col per tile and the offsets from it: (cbase, offsets, every
    offset fits in 16 bits).'''
    k0, k1 = p.tile_k()
    c = p.cols.astype(numpy.int64)
    cbase = numpy.array([c[a:b].min() for a, b in zip(k0, k1)])
    off = c - numpy.repeat(cbase, k1 - k0)
    return cbase, off, bool(off.max() <= 0xffff)


def packed_words(w16, off):
    '''(offset << 16) | half bits: the packed streams.'''
    bits = numpy.asarray(w16, dtype=numpy.float16).view(numpy.uint16)
    return ((off.astype(numpy.uint32) & 0xffff) << 16) | bits.astype(numpy.uint32)


def xcd_tile(b, nwg):
    '''common.h: the tile workgroup b of nwg takes (a bijection).'''
    group = 8 * XCD_RUN
    full = (nwg // group) * group
    if b < full:
        g, i = divmod(b, group)
        return g * group + (i & 7) * XCD_RUN + (i >> 3)
    nt, i = nwg - full, b - full
    q, r, xcd = nt >> 3, nt & 7, i & 7
    first = xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q
    return full + first + (i >> 3)


def cheb_coefficients(lo, hi, count):
    '''Cheb of csr_stream16.h: first() and `count` times next(), as the floats
    the kernels get.'''
    theta, delta = 0.5 * (hi + lo), 0.5 * (hi - lo)
    sigma = theta / delta
    rho = 1.0 / sigma
    c0 = numpy.float32(1.0 / theta)
    steps = []
    for _ in range(count):
        rn = 1.0 / (2.0 * sigma - rho)
        steps.append((numpy.float32(rn * rho), numpy.float32(2.0 * rn / delta)))
        rho = rn
    return c0, steps


# -- the product ----------------------------------------------------------------
def _columns(a, dtype):
    '''(m,) or (m, 2) -> (m, ncomp) of dtype.'''
    a = numpy.asarray(a).astype(dtype)
    return a.reshape(len(a), -1)


def blocked(a, n):
    '''Component-blocked (2n: the device's idrows, rowmask, fp64 vectors) ->
    (n, 2).'''
    return numpy.asarray(a).reshape(2, n).T


def _identity(idrows, mask, n):
    '''(n, k) bool: rows whose sum is the row's own g.  idrows: 1 = identity
    (flow_pmg_level.idrows); mask: 0 = identity (flow_operator.rowmask); both
    per row (n,) or per row and component (n, 2).'''
    ident = numpy.zeros((n, 1), dtype=bool)
    if idrows is not None:
        ident = ident | (numpy.asarray(idrows).reshape(n, -1) != 0)
    if mask is not None:
        ident = ident | (numpy.asarray(mask).reshape(n, -1) == 0)
    return ident


def tile_product(rowptr, cols, w, g, idrows=None, mask=None):
    '''s_i = sum_k w_k g[cols_k] over the nonzeros of row i, and per row
    sum_k |w_k| |g[cols_k]|, in float64.  w: the fp16-rounded weights, (nnz,)
    or one per component (nnz, 2); g: (n,) or (n, 2).  Identity rows (see
    _identity; flags per row or per row and component) return the row's own
    g.'''
    rp = numpy.asarray(rowptr, dtype=numpy.int64)
    n = len(rp) - 1
    g2 = _columns(g, numpy.float64)
    t = _columns(w, numpy.float64) * g2[numpy.asarray(cols, dtype=numpy.int64)]
    row_of = numpy.repeat(numpy.arange(n), numpy.diff(rp))
    s = numpy.zeros((n, t.shape[1]))
    sabs = numpy.zeros((n, t.shape[1]))
    numpy.add.at(s, row_of, t)
    numpy.add.at(sabs, row_of, numpy.abs(t))
    ident = numpy.broadcast_to(_identity(idrows, mask, n), s.shape)
    s = numpy.where(ident, g2, s)
    sabs = numpy.where(ident, numpy.abs(g2), sabs)
    shape = numpy.shape(g)
    return s.reshape(shape), sabs.reshape(shape)


def tile_product_f32(rowptr, cols, w, g, idrows=None, mask=None):
    '''The same sum as the kernel does it without FMA: fp32 products added in
    the order of the row's nonzeros.'''
    rp = numpy.asarray(rowptr, dtype=numpy.int64)
    n = len(rp) - 1
    cols = numpy.asarray(cols, dtype=numpy.int64)
    g2 = _columns(g, numpy.float32)
    w2 = _columns(w, numpy.float32)
    lens = numpy.diff(rp)
    s = numpy.zeros((n, g2.shape[1]), dtype=numpy.float32)
    order = numpy.argsort(-lens, kind='stable')
    for j in range(int(lens.max())):
        rows = order[:int((lens > j).sum())]
        k = rp[rows] + j
        s[rows] = s[rows] + w2[k] * g2[cols[k]]
    ident = numpy.broadcast_to(_identity(idrows, mask, n), s.shape)
    return numpy.where(ident, g2, s).reshape(numpy.shape(g))


def row_bound(lens, terms):
    '''(len + 4) 2^-24 (sum of the absolute values of the terms of the row's
    expression); lens per row, terms (n,) or (n, ncomp).'''
    lens = numpy.asarray(lens, dtype=numpy.float64)
    terms = numpy.asarray(terms, dtype=numpy.float64)
    if terms.ndim == 2:
        lens = lens[:, None]
    return (lens + 4.0) * U32 * terms


def worst_ratio(got, ref, bound):
    '''max over ALL rows of |got - ref| / bound (a zero bound asks for
    equality), and the row where it occurs.'''
    got = numpy.asarray(got, dtype=numpy.float64)
    err = numpy.abs(got - numpy.asarray(ref, dtype=numpy.float64))
    bound = numpy.broadcast_to(numpy.asarray(bound, dtype=numpy.float64),
                               err.shape)
    assert got.shape == err.shape and numpy.isfinite(bound).all()
    with numpy.errstate(divide='ignore', invalid='ignore'):
        ratio = numpy.where(bound > 0.0, err / bound,
                            numpy.where(err == 0.0, 0.0, numpy.inf))
    ratio = numpy.where(numpy.isfinite(got), ratio, numpy.inf)
    at = numpy.unravel_index(int(numpy.argmax(ratio)), ratio.shape)
    return float(ratio[at]), at


RATIOS = {}


def assert_rows(got, ref, bound, what):
    '''The comparator: every row within its bound.  Returns the worst
    error / bound and keeps it in RATIOS[what] for the report.'''
    worst, at = worst_ratio(got, ref, bound)
    RATIOS[what] = max(worst, RATIOS.get(what, 0.0))
    print('%-60s worst error / bound = %.3g' % (what, worst))
    assert worst <= 1.0, (
        '%s: row %s is off by %.3g times its bound (got %r, expected %r)'
        % (what, at, worst, numpy.asarray(got)[at], numpy.asarray(ref)[at]))
    return worst


# -- one launch of mass_cheb_kernel -----------------------------------------------
# mass_mode0 / mass_step: [(name, expected, bound)] for what the launch writes,
# from the vectors the device read (widened exactly).  The expected d and acc
# are formed around the rho / d the device wrote (rho_dev, d_dev), so that each
# line checks ONE expression with its own bound.  The *_f32 twins evaluate the
# same expressions in fp32 as the kernel does without FMA: the stand-in for a
# device result in the host tests (`product`: the row sums to use).
def _wide(*arrays):
    return [numpy.asarray(a).astype(numpy.float64) for a in arrays]


def mass_mode0(rp, cols, w, mask, rho0, c, rho_dev, d_dev):
    '''MODE 0 (s = A~ rho0): rho_1 = rho0 - c0 s ; d_1 = (c1 c0) rho0 + c2 rho_1
    ; acc = c0 rho0 + d_1.'''
    c0, (c1, c2) = c
    c10 = float(numpy.float32(c1 * c0))     # a float product in the kernel
    c0, c2 = float(c0), float(c2)
    lens = numpy.diff(rp)
    own, rho_d, d_d = _wide(rho0, rho_dev, d_dev)
    s, sabs = tile_product(rp, cols, w, own, mask=mask)
    return [
        ('rho', own - c0 * s, row_bound(lens, numpy.abs(own) + abs(c0) * sabs)),
        ('d', c10 * own + c2 * rho_d,
         row_bound(lens, numpy.abs(c10 * own) + numpy.abs(c2 * rho_d))),
        ('acc', c0 * own + d_d,
         row_bound(lens, numpy.abs(c0 * own) + numpy.abs(d_d)))]


def mass_mode0_f32(rp, cols, w, mask, rho0, c, product=None):
    c0, (c1, c2) = c
    c10 = numpy.float32(c1 * c0)
    own = numpy.asarray(rho0).astype(numpy.float32)
    s = (product or tile_product_f32)(rp, cols, w, own, mask=mask)
    rho = own - c0 * s
    d = c10 * own + c2 * rho
    return dict(rho=rho, d=d, acc=c0 * own + d)


def mass_step(rp, cols, w, mask, g, rho_old, acc_old, c12, rho_dev=None,
              d_dev=None):
    '''MODE 1 (s = A~ g, g = the d before): rho' = rho_old - s ;
    d' = c1 g + c2 rho' ; acc' = acc_old + d'.  MODE 2 (rho_dev = None) leaves
    only z = acc_old + d'.'''
    c1, c2 = float(c12[0]), float(c12[1])
    lens = numpy.diff(rp)
    own, r_old, a_old = _wide(g, rho_old, acc_old)
    s, sabs = tile_product(rp, cols, w, own, mask=mask)
    if rho_dev is None:
        return [('z', a_old + c1 * own + c2 * (r_old - s),
                 row_bound(lens, numpy.abs(a_old) + numpy.abs(c1 * own)
                           + abs(c2) * (numpy.abs(r_old) + sabs)))]
    rho_d, d_d = _wide(rho_dev, d_dev)
    return [
        ('rho', r_old - s, row_bound(lens, numpy.abs(r_old) + sabs)),
        ('d', c1 * own + c2 * rho_d,
         row_bound(lens, numpy.abs(c1 * own) + numpy.abs(c2 * rho_d))),
        ('acc', a_old + d_d, row_bound(lens, numpy.abs(a_old) + numpy.abs(d_d)))]


def mass_step_f32(rp, cols, w, mask, g, rho_old, acc_old, c12, product=None):
    c1, c2 = c12
    own, r_old, a_old = [numpy.asarray(a).astype(numpy.float32)
                         for a in (g, rho_old, acc_old)]
    s = (product or tile_product_f32)(rp, cols, w, own, mask=mask)
    rho = r_old - s
    d = c1 * own + c2 * rho
    return dict(rho=rho, d=d, acc=a_old + d, z=a_old + d)


# -- one pass of the power iteration (flow_pmg_lambda_max) ------------------------
def power_pass(rp, cols, w, v0, idrows=None):
    '''w1 = -(A~ v0) / |A~ v0| as (expected, bound): the row's product, one
    scalar multiply with float(1 / norm), and the relative error of the norm,
    4 * 2^-24 |expected|.  Of the latter one rounding is the float cast of
    1 / norm; the rest is what the rows' rounding errors e_i leave in the norm,
    to first order sum_i s_i e_i / |s|^2: hundreds of independent signed terms,
    O(u / sqrt(n)), as long as no single row carries the norm -- the absolute
    row sums are O(1) by construction (Pattern._values).'''
    lens = numpy.diff(rp)
    s, sabs = tile_product(rp, cols, w, v0, idrows=idrows)
    a = float(numpy.float32(1.0 / numpy.linalg.norm(s)))
    ref = -s * a
    return ref, row_bound(lens, sabs) * a + 4.0 * U32 * numpy.abs(ref)


def power_pass_f32(rp, cols, w, v0, idrows=None, product=None):
    s = (product or tile_product_f32)(rp, cols, w, v0, idrows=idrows)
    nrm = numpy.sqrt(numpy.sum(s.astype(numpy.float64)**2))
    return (numpy.float32(0.0) - s) * numpy.float32(1.0 / nrm)


def norm_of_product(rp, cols, w, v, idrows=None):
    '''|A~ v| and its tolerance: | |got| - |ref| | <= |got - ref|_2 <= the
    2-norm of the rows' bounds (the device sums the squares in fp64).'''
    lens = numpy.diff(rp)
    s, sabs = tile_product(rp, cols, w, v, idrows=idrows)
    ref = float(numpy.linalg.norm(s))
    return ref, float(numpy.linalg.norm(row_bound(lens, sabs))) + 1e-12 * ref
