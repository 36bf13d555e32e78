# -*- coding: utf-8 -*-
'''
CPU tests of the host model of the multicolour ILU(0) (tests/ilu_reference.py)
that tests/test_ilu_entries_gpu.py holds the kernels against: the model has the
defining property of ILU(0) on every case, reproduces a dense LU on a full
pattern, restates the pivot guard, and its float64 run stays within a small
multiple of eps64 * budget of its longdouble run (C_ref: printed, and asserted
finite and below 64 so that a broken reference is noticed).  The structure
every case is there for -- which factor kernel its longest row selects, the
slices per colour, the widths of the sweep streams -- is asserted from
plan.host alone; the GPU tests repeat those assertions.

Needs the library's host routines only (the colouring), no GPU.
'''
import numpy
import pytest

import ilu_reference as ir

CASES = ('fan15', 'fan16', 'fan20', 'square', 'strip')


@pytest.fixture(scope='module', autouse=True)
def colouring():
    from flow_amd import _hip
    try:
        _hip.load_library()
    except _hip.HipError as exc:
        pytest.skip('the host colouring routine of the library is not built: '
                    '%s' % exc)


def _product_on_pattern(host, lu):
    '''(L U)_ij at every position of the pattern, in longdouble (L with its
    unit diagonal; row k of U from its pivot on).'''
    rowptr, cols, diag = host['rowptr'], host['cols'], host['diag']
    n = len(rowptr) - 1
    upper = [{int(cols[q]): q for q in range(diag[k], rowptr[k + 1])}
             for k in range(n)]
    out = numpy.zeros(len(cols), dtype=numpy.longdouble)
    for i in range(n):
        for t in range(rowptr[i], rowptr[i + 1]):
            j = int(cols[t])
            s = numpy.longdouble(0.0)
            for p in range(rowptr[i], diag[i]):
                q = upper[int(cols[p])].get(j)
                if q is not None:
                    s += lu[p] * lu[q]
            if j >= i:
                s += lu[t]
            out[t] = s
    return out


@pytest.mark.parametrize('name', CASES)
def test_structure_of_the_cases(name):
    ir.check_structure(ir.plan_of(name), ir.STRUCTURES[name])
    got = ir.STRUCTURES[name]
    if name in ir.FANS:
        k = ir.FANS[name]
        assert got.max_row == got.n == 3 * k + 1 and got.longest_l == 3 * k
        # the hub's L row: several batches of both sweep kernels and a rest
        assert got.l_widths[-1] == 3 * k
        for batch in (ir.BATCH_FP64, ir.BATCH_PACKED):
            assert 3 * k >= 3 * batch and (3 * k % batch != 0) == (k == 15)
        assert got.kernel == ('sub' if k == 15 else 'scalar')
        if k == 15:
            # the sixth register slot of the eight-lane kernel, partly filled
            assert 5 * 8 < got.max_row < ir.SUB_KERNEL_MAX_ROW
        if k == 16:
            assert got.max_row == ir.SUB_KERNEL_MAX_ROW + 1
    else:
        assert got.kernel == 'sub'
        # a sweep launch of 2 or more workgroups, with a partial last slice
        # behind full ones
        plan = ir.plan_of(name)
        rows = numpy.diff(plan.colour_ptr)
        many = numpy.array(got.slices) > ir.SLICES_PER_WORKGROUP
        assert many.any() and (rows[many] % ir.SLICE != 0).any()
    if name == 'strip':
        # a slice wider than one batch of the fp64 sweep, with a rest, in a
        # launch of two workgroups
        assert got.slices[-1] > ir.SLICES_PER_WORKGROUP
        assert got.l_widths[-1] > ir.BATCH_FP64
        assert got.l_widths[-1] % ir.BATCH_FP64 != 0
        r0, r1 = ir.STRIP_ROWS
        c = ir.case(name)
        assert r0 % 64 and r1 % 64
        for cut in (r0, r1):       # couplings cross both cuts
            below = c.cols[c.rowptr[cut - 1]:c.rowptr[cut]]
            assert below.max() >= cut
            above = c.cols[c.rowptr[cut]:c.rowptr[cut + 1]]
            assert above.min() < cut


@pytest.mark.parametrize('name', CASES)
def test_source_positions_gather_the_permuted_block(name):
    '''src_pos against an independent search of every entry: the strip plan
    reads the diagonal block A[r0:r1, r0:r1] out of the full value planes.'''
    c, plan = ir.case(name), ir.plan_of(name)
    for plane in c.planes:
        want = ir.block_values(c.rowptr, c.cols, plane, plan.host, c.rows)
        assert numpy.array_equal(plane[plan.host['src_pos']], want)


@pytest.mark.parametrize('name', CASES)
def test_factor_reproduces_the_matrix_on_the_pattern(name):
    '''Defining property of ILU(0): (L U)_ij = a_ij at every position of the
    pattern, to 64 eps_longdouble * budget.'''
    plan = ir.plan_of(name)
    for block in (0, 1):
        ref = ir.factor_reference(name, block)
        assert ref['guarded'] == [] and ref['guarded64'] == []
        got = _product_on_pattern(plan.host, ref['lu80'])
        # (the budget of an L entry is in units of l_ik: times |u_kk| here)
        bud = ref['bud'].copy()
        h = plan.host
        for i in range(plan.n):
            for p in range(h['rowptr'][i], h['diag'][i]):
                bud[p] *= abs(ref['lu80'][h['diag'][h['cols'][p]]])
        err = abs(got - numpy.asarray(ref['vals'], dtype=numpy.longdouble))
        assert (err <= 64 * ir.EPS80 * bud).all(), \
            float((err / (ir.EPS80 * bud)).max())


def test_full_pattern_gives_the_dense_lu():
    '''On a full pattern ILU(0) is LU: L U = A everywhere.'''
    n = 12
    rng = numpy.random.RandomState(2)
    A = rng.standard_normal((n, n))
    A += numpy.diag(abs(A).sum(axis=1) + 1.0)
    host = {'rowptr': numpy.arange(n + 1, dtype=numpy.int32) * n,
            'cols': numpy.tile(numpy.arange(n, dtype=numpy.int32), n),
            'diag': (numpy.arange(n) * (n + 1)).astype(numpy.int32)}
    ref = ir.reference_of(ir.update_lists(host), A.ravel())
    lu = ref['lu80'].reshape(n, n)
    L = numpy.tril(lu, -1) + numpy.eye(n, dtype=numpy.longdouble)
    U = numpy.triu(lu)
    LU = numpy.array([[(L[i, :] * U[:, j]).sum() for j in range(n)]
                      for i in range(n)])
    mag = numpy.array([[abs(L[i, :] * U[:, j]).sum() for j in range(n)]
                       for i in range(n)])
    assert (abs(LU - A) <= 64 * ir.EPS80 * mag).all()
    assert numpy.isfinite(ref['c_ref']) and ref['c_ref'] < 64
    # ... and the sweeps then solve A z = r
    r = rng.standard_normal(n)
    dinv = 1.0 / ref['lu64'][host['diag']]
    z80, bud, _, _ = ir.sweeps(host, ref['lu64'], dinv, r, numpy.longdouble)
    A64 = (numpy.tril(ref['lu64'].reshape(n, n), -1) + numpy.eye(n)) \
        @ numpy.triu(ref['lu64'].reshape(n, n))
    assert abs(A64 @ z80.astype(numpy.float64) - r).max() < 1e-13


@pytest.mark.parametrize('name', ('fan15', 'fan16'))
@pytest.mark.parametrize('variant', ir.GUARD_VARIANTS)
def test_guard_restatement(name, variant):
    '''Guarded pivots equal their replacement bit for bit; the control, whose
    eliminated pivot is 2^-20 of the original, is left alone.'''
    plan = ir.plan_of(name)
    plane, pd, pivot, guarded = ir.guard_planes(name, variant)
    vals = plane[plan.host['src_pos']]
    ref = ir.reference_of(ir.lists_of(name), vals)
    hub = plan.n - 1
    for key, rows in (('lu80', ref['guarded']), ('lu64', ref['guarded64'])):
        assert rows == ([hub] if guarded else [])
        assert float(ref[key][pd]) == pivot
    replacement = vals[pd] if vals[pd] != 0.0 else 1.0
    assert (pivot == replacement) == guarded
    # a NaN pivot counts as collapsed
    bad = vals.copy()
    bad[plan.host['rowptr'][hub]] = numpy.nan
    lu, _, rows = ir.factor(ir.lists_of(name), bad, numpy.float64)
    assert hub in rows and lu[pd] == replacement


@pytest.mark.parametrize('name', CASES)
def test_float64_against_longdouble(name, capsys):
    '''C_ref of the factor and of the sweeps (all three arithmetic models):
    what the GPU tests scale their bounds with.'''
    c, plan = ir.case(name), ir.plan_of(name)
    h = plan.host
    line = [name]
    for block in (0, 1):
        ref = ir.factor_reference(name, block)
        assert numpy.isfinite(ref['c_ref']) and ref['c_ref'] < 64
        line.append('factor[%d] C_ref %.2f' % (block, ref['c_ref']))
        lu = ref['lu64']
        dinv = 1.0 / lu[h['diag']]
        rhs = c.rhs(plan.n, 2)[block][h['old_of_new']]
        for label, kw in (('fp64', {}), ('packed', {'packed': True}),
                          ('single', {'packed': True, 'single': True})):
            sw = ir.sweep_reference(h, lu, dinv, rhs, **kw)
            assert numpy.isfinite(sw['c_ref']) and sw['c_ref'] < 64
            line.append('%s C_ref %.2f' % (label, sw['c_ref']))
    with capsys.disabled():
        print('\n  ' + '  '.join(line))
