# -*- coding: utf-8 -*-
'''
Host model of the multicolour ILU(0) (helper, not a test): the factorisation
and the two sweeps of flow_amd/csrc/ilu_kernels.hip restated as plain loops
over the colour-permuted CSR of a plan (flow_amd/fem/ilu.py: IluPlan.host),
each in numpy.longdouble (the reference) and in numpy.float64 (what a correct
fp64 implementation of the same recurrence achieves), plus the cases of
tests/test_ilu_entries_host.py and tests/test_ilu_entries_gpu.py.

Why entry by entry: the suite sees the ILU almost only through a Krylov method,
and a Krylov method forgives a factor with a missed update -- it converges,
only more slowly.  Here every entry of the factor and every row of a sweep is
compared with the reference, against a budget of its own:

  factor   bud_t = |a_t| + sum |l_ik| |u_kj| over the updates entry t received
           (U and diagonal entries); the same divided by |u_kk| for an L entry
           l_ik.  The entry is the in-order evaluation of a_t - sum l_ik u_kj
           [/ u_kk]: every rounding of a correct implementation, in whatever
           order and with or without contraction to FMA, is a small multiple
           of eps * bud_t, to first order, plus what the operands (entries of
           earlier rows) carry.  What they carry is measured, not guessed:
           C_ref = max_t |lu64_t - lu80_t| / (eps64 bud_t) from the two host
           runs.  The device must stay within 8 max(1, C_ref) eps64 bud_t.  One
           missed or doubled update moves its entry by |l_ik u_kj|, a term OF
           the budget: ~1e13 times the bound on the cases here.
  sweeps   bud_i = |rhs_i| + sum |v_ik| |y_k| per row, times |1 / u_ii| in the
           backward sweep, the same way with C_ref of the sweeps.

The pivot guard is restated exactly: compare against the row's ORIGINAL
diagonal, threshold 1e-12, replacement d_orig or 1.0 when that is zero; a NaN
pivot counts as collapsed.

Cases: fans of k triangles around one hub vertex under P2 (the hub row holds
1 + 3 k entries: k = 15 fills the eight-lanes-per-row kernel's sixth register
slot partly, 16 is the first length that takes the one-lane-per-row kernel,
20 is well inside it), and UnitSquareMesh(20, 20, 'crossed') under P2, whose
colours have more than four slices (several workgroups per sweep launch).
'''
import contextlib
import ctypes
import functools

import numpy

EPS64 = float(numpy.finfo(numpy.float64).eps)
EPS32 = float(numpy.finfo(numpy.float32).eps)
EPS80 = float(numpy.finfo(numpy.longdouble).eps)

# the dispatch of factor() in ilu_kernels.hip: kSub * kSlots
SUB_KERNEL_MAX_ROW = 48
SLICE = 64
# slices a workgroup of the sweep kernels takes (kBlock / kSlice)
SLICES_PER_WORKGROUP = 4
# entries per lane and batch: ilu_sweep_kernel, ilu_sweep_packed_kernel
BATCH_FP64, BATCH_PACKED = 12, 4


# -- the model ----------------------------------------------------------------
def update_lists(host):
    '''The structure of IKJ ILU(0) on the permuted pattern, once per plan:
    for every row its (p0, pd, p1) and, per L entry p (ascending), the pivot
    position of row k = cols[p] and the pairs (t, q): entry t of row i
    receives - l_ik * u at position q of row k.'''
    rowptr = [int(x) for x in host['rowptr']]
    cols = [int(x) for x in host['cols']]
    diag = [int(x) for x in host['diag']]
    n = len(rowptr) - 1
    upper = [None] * n

    def upper_of(k):
        if upper[k] is None:
            upper[k] = {cols[q]: q for q in range(diag[k] + 1, rowptr[k + 1])}
        return upper[k]

    rows = []
    for i in range(n):
        p0, pd, p1 = rowptr[i], diag[i], rowptr[i + 1]
        assert p0 <= pd < p1 and cols[pd] == i
        assert all(cols[t] < cols[t + 1] for t in range(p0, p1 - 1))
        steps = []
        for p in range(p0, pd):
            k = cols[p]
            pos = upper_of(k)
            pairs = [(t, pos[cols[t]]) for t in range(p + 1, p1)
                     if cols[t] in pos]
            steps.append((p, diag[k], pairs))
        rows.append((pd, steps))
    return rows


def factor(rows, vals, dtype):
    '''ILU(0) of the values `vals` (permuted CSR order) in `dtype`.  Returns
    (lu, budget, guarded): the combined L\\U values, the budget of every
    entry (module docstring) and the rows whose pivot the guard replaced.'''
    v = [dtype(x) for x in vals]
    bud = [abs(x) for x in v]
    guarded = []
    threshold = dtype(1.0e-12)
    with numpy.errstate(all='ignore'):
        for i, (pd, steps) in enumerate(rows):
            d_orig = v[pd]
            for p, dk, pairs in steps:
                lik = v[p] / v[dk]
                v[p] = lik
                bud[p] = bud[p] / abs(v[dk])
                al = abs(lik)
                for t, q in pairs:
                    v[t] = v[t] - lik * v[q]
                    bud[t] = bud[t] + al * abs(v[q])
            d = v[pd]
            if not (abs(d) > threshold * abs(d_orig)):
                v[pd] = d_orig if d_orig != 0.0 else dtype(1.0)
                guarded.append(i)
    return (numpy.array(v, dtype=dtype), numpy.array(bud, dtype=dtype),
            guarded)


def ratio(got, ref, bud, eps):
    '''max |got - ref| / (eps * bud); an entry with budget 0 (a zero that no
    update touched) must be reproduced exactly.'''
    got = numpy.asarray(got, dtype=numpy.longdouble)
    ref = numpy.asarray(ref, dtype=numpy.longdouble)
    bud = numpy.asarray(bud, dtype=numpy.longdouble)
    err = abs(got - ref)
    assert numpy.isfinite(ref).all() and numpy.isfinite(bud).all()
    if not numpy.isfinite(err).all():
        return float('inf')
    zero = bud == 0
    if (err[zero] != 0).any():
        return float('inf')
    if zero.all():
        return 0.0
    return float((err[~zero] / (eps * bud[~zero])).max())


def sweeps(host, lu, dinv, rhs, dtype, packed=False, single=False):
    '''Forward (unit lower) and backward substitution with the combined factor
    values `lu` (permuted CSR) and the inverse pivots `dinv` as the kernels
    read them, on the permuted right-hand side `rhs`:
        y_i = rhs_i - sum_k l_ik y_k,   z_i = (y_i - sum_j u_ij z_j) dinv_i.
    packed: the L and U entries rounded to fp32 (the pivots' inverse stays
    fp64).  single (flow_ilu.single_vector): the input and every finished row
    rounded to fp32.  Returns (z, budget of z per row, y, budget of y).'''
    rowptr, cols, diag = host['rowptr'], host['cols'], host['diag']
    n = len(rowptr) - 1
    w = numpy.asarray(lu, dtype=numpy.float64)
    if packed:
        w = w.astype(numpy.float32).astype(numpy.float64)
    w = [dtype(x) for x in w]
    di = [dtype(x) for x in numpy.asarray(dinv, dtype=numpy.float64)]
    rhs = numpy.asarray(rhs, dtype=numpy.float64)
    finish = (lambda x: dtype(numpy.float32(x))) if single else (lambda x: x)
    if single:
        rhs = rhs.astype(numpy.float32).astype(numpy.float64)
    y = [dtype(x) for x in rhs]
    bud_y = [abs(x) for x in y]
    cols = [int(c) for c in cols]
    for i in range(n):
        s = dtype(0.0)
        b = bud_y[i]
        for p in range(rowptr[i], diag[i]):
            s = s + w[p] * y[cols[p]]
            b = b + abs(w[p]) * abs(y[cols[p]])
        y[i] = finish(y[i] - s)
        bud_y[i] = b
    # the right-hand side of the backward sweep is the forward result, known
    # to eps * bud_y only: that, not |y_i|, is its share of the budget (a row
    # of the last colour has no U part: z_i = y_i dinv_i, and where the forward
    # sum cancelled |y_i| says nothing about what a correct sweep can deliver)
    z = list(y)
    bud_z = list(bud_y)
    for i in range(n - 1, -1, -1):
        s = dtype(0.0)
        b = bud_z[i]
        for p in range(diag[i] + 1, rowptr[i + 1]):
            s = s + w[p] * z[cols[p]]
            b = b + abs(w[p]) * abs(z[cols[p]])
        z[i] = finish((z[i] - s) * di[i])
        bud_z[i] = b * abs(di[i])
    as_a = lambda a: numpy.array(a, dtype=dtype)
    return as_a(z), as_a(bud_z), as_a(y), as_a(bud_y)


def block_values(rowptr, cols, plane, plan_host, rows=None):
    '''The values of the diagonal block `rows` = (r0, r1) of a value plane over
    the ORIGINAL pattern (rowptr, cols), in the permuted CSR order of a plan,
    found by searching every entry -- independent of the plan's src_pos, which
    it checks (with the permuted pattern itself).'''
    n_all = len(rowptr) - 1
    r0, r1 = (0, n_all) if rows is None else rows
    old_of_new = plan_host['old_of_new']
    new_of_old = plan_host['new_of_old']
    p_rowptr, p_cols = plan_host['rowptr'], plan_host['cols']
    out = numpy.empty(len(p_cols), dtype=numpy.float64)
    assert len(old_of_new) == r1 - r0 == len(p_rowptr) - 1
    for i in range(r1 - r0):
        o = r0 + int(old_of_new[i])
        seg = slice(int(rowptr[o]), int(rowptr[o + 1]))
        c = numpy.asarray(cols[seg], dtype=numpy.int64)
        inside = (c >= r0) & (c < r1)
        new = new_of_old[c[inside] - r0]
        order = numpy.argsort(new)
        a, b = int(p_rowptr[i]), int(p_rowptr[i + 1])
        assert numpy.array_equal(new[order], p_cols[a:b]), i
        out[a:b] = numpy.asarray(plane[seg])[inside][order]
    return out


# -- meshes and values --------------------------------------------------------
def fan_mesh(k):
    '''k triangles around one hub vertex, the hub LAST: under P2 its dof is the
    last one and coupled to every other (N = 3 k + 1 = the hub row's length),
    so first-fit colouring gives it a colour of its own, the highest, and its
    whole row is L part.'''
    from flow_amd import fem
    phi = 2.0 * numpy.pi * numpy.arange(k) / k
    rim = numpy.stack([numpy.cos(phi), numpy.sin(phi)], axis=1)
    rim *= (1.0 + 0.15 * numpy.cos(3.0 * phi))[:, None]      # no two cells alike
    points = numpy.concatenate([rim, [[0.0, 0.0]]])
    cells = numpy.array([[k, j, (j + 1) % k] for j in range(k)],
                        dtype=numpy.int32)
    return fem.Mesh(points, cells, reorder=False)


class Structure(object):
    '''What a case is there for, asserted from plan.host alone by the host AND
    the GPU tests (a case cannot silently stop covering it).'''

    def __init__(self, n, max_row, longest_l, slices, l_widths, u_widths):
        self.n = n
        self.max_row = max_row
        self.kernel = 'sub' if max_row <= SUB_KERNEL_MAX_ROW else 'scalar'
        self.longest_l = longest_l        # L length of the longest row
        self.slices = slices              # per colour
        self.l_widths = l_widths          # per slice
        self.u_widths = u_widths


def structure_of(plan):
    h = plan.host
    length = numpy.diff(h['rowptr'])
    longest = int(numpy.argmax(length))
    l_len = h['diag'] - h['rowptr'][:-1]
    return Structure(
        plan.n, int(length.max()), int(l_len[longest]),
        [int(x) for x in numpy.diff(plan.slptr)],
        [int(x) // SLICE for x in numpy.diff(h['l_sl_off'])],
        [int(x) // SLICE for x in numpy.diff(h['u_sl_off'])])


def check_structure(plan, want):
    '''`want`: the Structure written down in CASES.'''
    got = structure_of(plan)
    assert plan.struct.max_row == got.max_row
    for key in ('n', 'max_row', 'kernel', 'longest_l', 'slices', 'l_widths',
                'u_widths'):
        assert getattr(got, key) == getattr(want, key), \
            (key, getattr(got, key), getattr(want, key))
    # the sweeps: rows without an L part (colour 0) and without a U part (the
    # last colour) -- slices of width 0 -- are part of every case
    assert got.l_widths[0] == 0 and got.u_widths[-1] == 0
    h = plan.host
    c0 = int(plan.colour_ptr[1])
    assert (h['diag'][:c0] == h['rowptr'][:c0]).all()
    last = int(plan.colour_ptr[-2])
    assert (h['diag'][last:] + 1 == h['rowptr'][last + 1:]).all()
    return got


def fan_structure(k, slices, l_widths, u_widths):
    return Structure(3 * k + 1, 3 * k + 1, 3 * k, slices, l_widths, u_widths)


class Case(object):
    '''A mesh under P2, two value planes over its pattern (mass + 0.002
    stiffness + a 10 % random perturbation on the pattern, drawn per plane),
    optionally a strip of rows (the block-Jacobi plan of flow_amd/parallel.py).
    Matrices of kind 0 / 1 / 2 take planes [0] / [0, 1] / [0, NaN, NaN, 1]:
    the factor reads planes 0 and 3 of a 2x2-block matrix, never the others.

    The perturbation is 10 % of the largest mass entry, as in
    tests/test_hip_ilu.py -- on a regular mesh, where every diagonal entry is
    of that size.  relative (the fans): 10 % of sqrt(m_ii m_jj) per entry.  A
    rim vertex of a fan belongs to two cells and the hub to all: the mass
    diagonal spans a factor 7, and 10 % of the largest entry on each of a rim
    row's ~12 entries leaves that row nearly singular (measured on fan 15:
    multipliers up to 44, C_ref = 282 -- a matrix on which ILU(0) itself is
    ill conditioned tells nothing about a kernel).'''

    def __init__(self, name, mesh, seed, rows=None, relative=False):
        from flow_amd.fem.space import scalar_layout
        from oracle import fem_oracle as orc
        self.name = name
        self.mesh = mesh
        self.rows = rows
        lay = self.layout = scalar_layout(mesh, 2)
        self.rowptr = lay.pattern('rowptr')
        self.cols = lay.pattern('cols')
        S = orc.Space(mesh.points, mesh.cell_vertices, lay.cell_dofs, 2, lay.N)
        M = pattern_values(orc.mass_matrix(S), self.rowptr, self.cols)
        K = pattern_values(orc.stiffness_matrix(S), self.rowptr, self.cols)
        rng = numpy.random.RandomState(seed)
        scale = abs(M).max()
        if relative:
            d = M[lay.pattern('diag_idx')]
            row_of = numpy.repeat(numpy.arange(lay.N), numpy.diff(self.rowptr))
            scale = numpy.sqrt(d[row_of] * d[self.cols])
        self.planes = [
            M + 0.002 * K + 0.1 * rng.standard_normal(len(M)) * scale
            for _ in range(2)]
        self.rhs_seed = seed + 100

    def all_planes(self, kind, blocks=None):
        '''The value planes of a Matrix of `kind` (host arrays).'''
        a, b = self.planes if blocks is None else blocks
        nan = numpy.full(len(a), numpy.nan)
        return {0: [a], 1: [a, b], 2: [a, nan, nan, b]}[kind]

    def blocks(self, kind, blocks=None):
        '''The planes the factor of a Matrix of `kind` reads, per block.'''
        a, b = self.planes if blocks is None else blocks
        return [a] if kind == 0 else [a, b]

    def rhs(self, n, nblocks):
        '''A different right-hand side per block (original numbering).'''
        rng = numpy.random.RandomState(self.rhs_seed)
        return rng.standard_normal((nblocks, n))


def pattern_values(M, rowptr, cols):
    '''The values of a scipy matrix in the order of a CSR pattern.'''
    M = M.tocsr()
    rows = numpy.repeat(numpy.arange(len(rowptr) - 1), numpy.diff(rowptr))
    return numpy.asarray(M[rows, cols]).ravel()


FANS = {'fan15': 15, 'fan16': 16, 'fan20': 20}
SQUARE_N = 20
# the strip: neither end a multiple of 64, couplings cross both cuts
STRIP_ROWS = (1003, 2411)

# The structures, read off the plans once and written down: slices per colour,
# then the widths of the L and of the U stream per slice.
STRUCTURES = {
    'fan15': fan_structure(15, [1] * 8, [0, 2, 3, 6, 7, 6, 7, 45],
                           [8, 6, 5, 4, 3, 2, 1, 0]),
    'fan16': fan_structure(16, [1] * 6, [0, 2, 3, 6, 7, 48],
                           [8, 6, 5, 2, 1, 0]),
    'fan20': fan_structure(20, [1] * 6, [0, 2, 3, 6, 7, 60],
                           [8, 6, 5, 2, 1, 0]),
    # colours of 839, 801, 221, 220, 800 and 400 rows
    'square': Structure(
        3281, 25, 10, [14, 13, 4, 4, 13, 7],
        [0] * 14 + [2] * 13 + [10] * 4 + [14] * 4 + [7] * 13 + [12] * 7,
        [5] + [8] * 13 + [6] * 13 + [14] * 4 + [10] * 4 + [1] * 13 + [0] * 7),
    # colours of 408, 397, 119, 118 and 366 rows
    'strip': Structure(
        1408, 21, 10, [7, 7, 2, 2, 6],
        [0] * 7 + [2] * 7 + [10, 10, 14, 15] + [7] * 5 + [20],
        [6] * 6 + [9] + [5] * 7 + [10, 10, 6, 6] + [0] * 6),
    }


@functools.lru_cache(maxsize=None)
def case(name):
    if name in FANS:
        return Case(name, fan_mesh(FANS[name]), 11 + FANS[name],
                    relative=True)
    if name == 'square':
        return Case(name, _square(), 5)
    assert name == 'strip'
    return Case(name, _square(), 6, rows=STRIP_ROWS)


@functools.lru_cache(maxsize=None)
def _square():
    from flow_amd import fem
    return fem.UnitSquareMesh(SQUARE_N, SQUARE_N, 'crossed')


@contextlib.contextmanager
def host_pointers():
    '''Let IluPlan build its struct over HOST tensors where there is no GPU:
    nothing is launched, only plan.host is looked at.'''
    from flow_amd import _hip, device
    if device.on_gpu():
        yield
        return

    def ptr(t, dtype, numel=None, name='operand'):
        if t is None:
            return None
        assert t.dtype == dtype and t.is_contiguous()
        assert numel is None or t.numel() >= numel
        return ctypes.c_void_p(t.data_ptr())
    keep = _hip._ptr
    _hip._ptr = ptr
    try:
        yield
    finally:
        _hip._ptr = keep


@functools.lru_cache(maxsize=None)
def plan_of(name):
    '''The plan of a case, as the product builds it: plan_for(layout), or
    IluPlan(layout, rows=...) for the strip (parallel.local_ilu).'''
    from flow_amd.fem import ilu
    c = case(name)
    with host_pointers():
        if c.rows is None:
            return ilu.plan_for(c.layout)
        return ilu.IluPlan(c.layout, rows=c.rows)


@functools.lru_cache(maxsize=None)
def lists_of(name):
    return update_lists(plan_of(name).host)


@functools.lru_cache(maxsize=None)
def factor_reference(name, block):
    '''dict of the two host factorisations of value plane `block` of a case:
    lu80, bud (longdouble), lu64, c_ref.  Once per session.'''
    c, plan = case(name), plan_of(name)
    vals = c.planes[block][plan.host['src_pos']]
    return reference_of(lists_of(name), vals)


def reference_of(rows, vals):
    lu80, bud, g80 = factor(rows, vals, numpy.longdouble)
    lu64, bud64, g64 = factor(rows, vals, numpy.float64)
    return {'vals': vals, 'lu80': lu80, 'bud': bud, 'lu64': lu64,
            'bud64': bud64, 'guarded': g80, 'guarded64': g64,
            'c_ref': ratio(lu64, lu80, bud, EPS64)}


def factor_bound(ref):
    '''Per entry: 8 max(1, C_ref) eps64 bud_t.'''
    return 8.0 * max(1.0, ref['c_ref']) * EPS64 * ref['bud']


def sweep_reference(host, lu, dinv, rhs, packed=False, single=False):
    '''Both host substitutions with the given factor: dict z80, bud, z64,
    c_ref and the eps of the variant (eps32 for single_vector).'''
    eps = EPS32 if single else EPS64
    z80, bud, _, _ = sweeps(host, lu, dinv, rhs, numpy.longdouble,
                            packed=packed, single=single)
    z64, _, _, _ = sweeps(host, lu, dinv, rhs, numpy.float64,
                          packed=packed, single=single)
    return {'z80': z80, 'bud': bud, 'z64': z64, 'eps': eps,
            'c_ref': ratio(z64, z80, bud, eps)}


# -- pivot guard cases ----------------------------------------------------------
GUARD_VARIANTS = ('collapse', 'zero_diagonal', 'control')


def guard_planes(name, variant):
    '''Value plane of a fan case with the hub row i (the one row of the last
    colour) rebuilt from powers of two: its L part zero except the coupling to
    one lower-coloured row k, the L part of row k zero as well.  k is the row
    just before the hub: its U part is the coupling to the hub alone, so
    eliminating it touches nothing but the pivot (no fill inside the pattern),
    every other multiplier of the two rows is 0 / u_jj = 0 and its updates
    subtract exact zeros, u_kk = a_kk and u_ki = a_ki are the matrix entries
    themselves, and the eliminated pivot is EXACTLY
        a_ii - (a_ik / a_kk) a_ki
    with or without contraction.
      collapse       a_kk = 2, a_ik = a_ki = 1, a_ii = 2^-1: pivot 0, replaced
                     by a_ii;
      zero_diagonal  a_kk = 2, a_ik = 1, a_ki = 0, a_ii = 0: pivot 0, replaced
                     by 1.0;
      control        a_kk = 1, a_ki = 1, a_ik = 1 - 2^-20, a_ii = 1: pivot
                     2^-20 a_ii, far above 1e-12 a_ii: stays.
    Returns (plane, position of the pivot in the permuted CSR, the value the
    factor must hold there, guarded or not).'''
    c, plan = case(name), plan_of(name)
    h = plan.host
    n = plan.n
    assert int(plan.colour_ptr[-2]) == n - 1       # the hub: alone, last
    i, k = n - 1, n - 2
    assert h['diag'][k] + 2 == h['rowptr'][k + 1]       # U part: the hub
    src = h['src_pos']
    plane = c.planes[1].copy()

    def pos(r, col):
        a, b = int(h['rowptr'][r]), int(h['rowptr'][r + 1])
        t = a + int(numpy.searchsorted(h['cols'][a:b], col))
        assert h['cols'][t] == col
        return t
    pd = int(h['diag'][i])
    assert pd == int(h['rowptr'][i + 1]) - 1       # the whole row is L part
    a_kk, a_ik, a_ki, a_ii, pivot, guarded = {
        'collapse': (2.0, 1.0, 1.0, 0.5, 0.5, True),
        'zero_diagonal': (2.0, 1.0, 0.0, 0.0, 1.0, True),
        'control': (1.0, 1.0 - 2.0**-20, 1.0, 1.0, 2.0**-20, False),
        }[variant]
    plane[src[int(h['rowptr'][i]):pd]] = 0.0
    plane[src[int(h['rowptr'][k]):int(h['diag'][k])]] = 0.0
    plane[src[pos(i, k)]] = a_ik
    plane[src[pos(k, k)]] = a_kk
    plane[src[pos(k, i)]] = a_ki
    plane[src[pd]] = a_ii
    return plane, pd, pivot, guarded
