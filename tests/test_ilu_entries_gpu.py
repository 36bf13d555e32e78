# -*- coding: utf-8 -*-
'''
K11, entry by entry: the multicolour ILU(0) of flow_amd/csrc/ilu_kernels.hip
through ilu.Ilu0 and the C ABI against the host model of
tests/ilu_reference.py (bounds and cases: its docstring; the model itself is
checked by tests/test_ilu_entries_host.py).

  * both factor kernels -- eight lanes per row (rows up to 48 entries: fan 15
    with its sixth register slot partly filled, the square, the strip) and one
    lane per row (fan 16, fan 20) --, one and two blocks, every entry against
    the longdouble factor;
  * the pivot guard of both, from powers of two;
  * the split into sweep streams, the inverse pivots and the fp32 packing, bit
    for bit;
  * the fp64, packed and single-vector sweeps per row, with the factor read
    back from the device, on launches of several workgroups and on the hub's L
    row of 45 / 48 / 60 entries (batches of 12 and 4 with a rest);
  * the block-Jacobi plan of a strip (flow_amd/parallel.py: local_ilu);
  * refactor() against a fresh factorisation.
Every test repeats the structure assertions of its case: which kernel the
longest row selects, slices per colour, widths.
'''
import numpy
import pytest

import ilu_reference as ir

pytestmark = pytest.mark.gpu

CASES = ('fan15', 'fan16', 'fan20', 'square', 'strip')


def _plan(name):
    plan = ir.plan_of(name)
    got = ir.check_structure(plan, ir.STRUCTURES[name])
    want = {'fan15': 'sub', 'fan16': 'scalar', 'fan20': 'scalar',
            'square': 'sub', 'strip': 'sub'}[name]
    assert got.kernel == want
    # what factor() in ilu_kernels.hip dispatches on
    assert (plan.struct.max_row > ir.SUB_KERNEL_MAX_ROW) == (want == 'scalar')
    return plan


def _matrix(case, kind, blocks=None):
    from flow_amd import device
    from flow_amd.fem import ops
    planes = case.all_planes(kind, blocks)
    return ops.Matrix(case.layout, kind,
                      device.to_device(numpy.concatenate(planes)))


def _ilu(name, kind, blocks=None, **kw):
    '''As flow_amd/parallel.py builds it: the case's plan handed to Ilu0.'''
    from flow_amd.fem import ilu
    plan = _plan(name)
    return ilu.Ilu0(_matrix(ir.case(name), kind, blocks), plan=plan, **kw), plan


def _buffers(pre):
    '''Host copies of the factor buffer per block: combined values, L stream,
    U stream, inverse pivots.'''
    from flow_amd import device
    plan = pre.plan
    lu = device.to_host(pre.lu).numpy()
    out = []
    for b in range(len(pre.planes)):
        base = lu[b * plan.lu_size:(b + 1) * plan.lu_size]
        out.append({
            'lu': base[:plan.nnz],
            'l': base[plan.off_l:plan.off_l + plan.nnz_l],
            'u': base[plan.off_u:plan.off_u + plan.nnz_u],
            'dinv': base[plan.off_d:plan.off_d + plan.n],
            })
    return out


def _bits(a):
    a = numpy.ascontiguousarray(a)
    return a.view({4: numpy.int32, 8: numpy.int64}[a.dtype.itemsize])


def _check_factor(label, got, ref):
    achieved = ir.ratio(got, ref['lu80'], ref['bud'], ir.EPS64)
    print('%s: factor C_ref %.2f, device %.2f (bound %.1f)'
          % (label, ref['c_ref'], achieved, 8.0 * max(1.0, ref['c_ref'])))
    err = abs(numpy.asarray(got, dtype=numpy.longdouble) - ref['lu80'])
    assert (err <= ir.factor_bound(ref)).all(), (label, achieved)


@pytest.mark.parametrize('kind', [0, 1, 2])
@pytest.mark.parametrize('name', CASES)
def test_factor_entries(hip, name, kind):
    '''Every entry of every block against the longdouble ILU(0) of the
    permuted pattern.  Kind 2: planes 1 and 2 hold NaN -- the factor reads
    planes 0 and 3 only.'''
    pre, plan = _ilu(name, kind)
    c = ir.case(name)
    bufs = _buffers(pre)
    assert len(bufs) == (1 if kind == 0 else 2)
    for b, buf in enumerate(bufs):
        ref = ir.factor_reference(name, b)
        if c.rows is not None:
            # the strip: the diagonal block A[r0:r1, r0:r1] of the full plane
            assert numpy.array_equal(ref['vals'], ir.block_values(
                c.rowptr, c.cols, c.planes[b], plan.host, c.rows))
        assert ref['guarded'] == []
        _check_factor('%s kind %d block %d' % (name, kind, b), buf['lu'], ref)


@pytest.mark.parametrize('variant', ir.GUARD_VARIANTS)
@pytest.mark.parametrize('nb', [1, 2])
@pytest.mark.parametrize('name', ['fan15', 'fan16'])
def test_pivot_guard(hip, name, nb, variant):
    '''Both kernels, one and two blocks: a pivot that collapses to exactly 0
    is replaced by the row's original diagonal, by 1.0 where that is zero; a
    pivot of 2^-20 of the original stays.  With two blocks only block 1
    collapses: block 0 is its unguarded factor.'''
    c = ir.case(name)
    plane, pd, pivot, guarded = ir.guard_planes(name, variant)
    pre, plan = _ilu(name, nb - 1, blocks=(plane, plane) if nb == 1
                     else (c.planes[0], plane))
    bufs = _buffers(pre)
    vals = plane[plan.host['src_pos']]
    ref = ir.reference_of(ir.lists_of(name), vals)
    assert ref['guarded'] == ([plan.n - 1] if guarded else [])
    got = bufs[-1]['lu']
    assert _bits(got[pd:pd + 1])[0] == _bits(numpy.array([pivot]))[0], got[pd]
    replacement = vals[pd] if vals[pd] != 0.0 else 1.0
    assert (got[pd] == replacement) == guarded
    assert bufs[-1]['dinv'][plan.n - 1] == 1.0 / pivot
    _check_factor('%s %s nb %d guarded block' % (name, variant, nb), got, ref)
    if nb == 2:
        ref0 = ir.factor_reference(name, 0)
        assert ref0['guarded'] == []
        _check_factor('%s %s block 0' % (name, variant), bufs[0]['lu'], ref0)


@pytest.mark.parametrize('nb', [1, 2])
@pytest.mark.parametrize('name', ['fan16', 'square', 'strip'])
def test_split_and_pack(hip, name, nb):
    '''The sweep streams are the factor entries at l_pos / u_pos bit for bit
    with +0.0 at every pad position, dinv is 1 / pivot to 1 ulp, the packed
    buffer float32(stream) with the blocks interleaved, U behind L.'''
    from flow_amd import device
    pre, plan = _ilu(name, {1: 0, 2: 2}[nb], packed=True)
    h = plan.host
    bufs = _buffers(pre)
    packed = device.to_host(pre.packed).numpy()
    assert packed.dtype == numpy.float32
    assert len(packed) == (plan.nnz_l + plan.nnz_u) * nb + 4
    for b, buf in enumerate(bufs):
        for key, pos, count, at in (('l', h['l_pos'], plan.nnz_l, 0),
                                    ('u', h['u_pos'], plan.nnz_u,
                                     plan.nnz_l * nb)):
            pos = pos[:count]
            assert (pos == -1).any() and (pos >= 0).any()
            want = numpy.where(pos >= 0, buf['lu'][numpy.maximum(pos, 0)], 0.0)
            assert numpy.array_equal(_bits(buf[key]), _bits(want)), (b, key)
            want32 = want.astype(numpy.float32)
            got32 = packed[at + b:at + count * nb:nb]
            assert numpy.array_equal(_bits(got32), _bits(want32)), (b, key)
        exact = 1.0 / buf['lu'][h['diag']]
        assert (abs(buf['dinv'] - exact) <= numpy.spacing(abs(exact))).all()
    assert (packed[-4:] == 0.0).all()


SWEEPS = {'fp64': {}, 'packed': {'packed': True},
          'single': {'packed': True, 'single_vector': True}}


@pytest.mark.parametrize('nb', [1, 2])
@pytest.mark.parametrize('variant', sorted(SWEEPS))
@pytest.mark.parametrize('name', CASES)
def test_sweep_rows(hip, name, variant, nb):
    '''flow_ilu0_solve per row, in the permuted numbering, against
    substitution in longdouble with the factor read back from the device: the
    sweeps alone, whatever the factor kernels did.  packed: the reference
    applies the fp32-rounded entries; single: it also rounds the input and
    every finished row to fp32, and eps32 takes the place of eps64.  A
    different right-hand side per block; two applications agree bit for bit.'''
    from flow_amd import device
    kw = SWEEPS[variant]
    pre, plan = _ilu(name, {1: 0, 2: 2}[nb], **kw)
    h = plan.host
    n = plan.n
    r = ir.case(name).rhs(n, nb)
    rd = device.to_device(r.ravel())
    z = device.to_host(pre.solve(rd, device.zeros(nb * n))).numpy()
    again = device.to_host(pre.solve(rd, device.zeros(nb * n))).numpy()
    assert numpy.array_equal(_bits(z), _bits(again))
    assert numpy.isfinite(z).all()
    perm = h['old_of_new']
    for b, buf in enumerate(_buffers(pre)):
        ref = ir.sweep_reference(
            h, buf['lu'], buf['dinv'], r[b][perm], packed='packed' in kw,
            single='single_vector' in kw)
        assert numpy.isfinite(ref['c_ref']) and ref['c_ref'] < 64
        got = z[b * n:(b + 1) * n][perm]
        achieved = ir.ratio(got, ref['z80'], ref['bud'], ref['eps'])
        print('%s %s nb %d block %d: sweeps C_ref %.2f, device %.2f'
              % (name, variant, nb, b, ref['c_ref'], achieved))
        bound = 8.0 * max(1.0, ref['c_ref']) * ref['eps'] * ref['bud']
        err = abs(numpy.asarray(got, dtype=numpy.longdouble) - ref['z80'])
        assert (err <= bound).all(), achieved


@pytest.mark.parametrize('name', ['fan15', 'fan16', 'square'])
def test_refactor_equals_a_fresh_factorisation(hip, name):
    '''refactor(A2) on an Ilu0 that holds the factors of A1 leaves the same
    factor buffer and the same packed streams, bit for bit, as Ilu0(A2): the
    kernels carry nothing over.'''
    from flow_amd import device
    c = ir.case(name)
    second = (1.5 * c.planes[1], 0.75 * c.planes[0])
    pre, _ = _ilu(name, 1, packed=True)
    pre.refactor(_matrix(c, 1, second))
    fresh, _ = _ilu(name, 1, blocks=second, packed=True)
    for key in ('lu', 'packed'):
        a = device.to_host(getattr(pre, key)).numpy()
        b = device.to_host(getattr(fresh, key)).numpy()
        assert numpy.isfinite(a).all()
        assert numpy.array_equal(_bits(a), _bits(b)), key
