# -*- coding: utf-8 -*-
'''
What the trajectory comparison of tests/test_krylov_trajectories_gpu.py can
see (CPU only; tests/krylov_reference.py).  On the cases whose matrices can be
built without the library (assembled by oracle/fem_oracle.py on the same
meshes; no preconditioner, Jacobi, and a two-level map over 3 x 3 bins):

  * the tolerance of every case, measured reference against reference (the
    textbook algorithm in fp64 against extended precision) -- never against
    device output; the fp64 run stays within tol / 100 by construction;
  * the conditions the systems were chosen for: >= 6 compared iterates above
    the residual floor, two full cycles and a partial one for the GMRES
    restart cases, the kept and dropped starts, the factor-10 gap at k* of
    the counts with estimate and true residual within 1 %;
  * every mutant of the reference departs from it by >= 1000 tolerances.
'''
import functools

import numpy
import pytest

import krylov_reference as kr

BIG = (512, 512)          # P1 on a rectangle: 513^2 = 263169 > 262144, odd


def _pattern(mesh, deg, with_stiffness):
    from flow_amd import fem
    from oracle import fem_oracle as orc
    V = fem.FunctionSpace(mesh, 'CG', deg)
    lay = V.layout
    rp = numpy.asarray(lay.pattern('rowptr'), dtype=numpy.int64)
    ci = numpy.asarray(lay.pattern('cols'), dtype=numpy.int64)
    S = orc.Space(mesh.points, mesh.cell_vertices, lay.cell_dofs, deg, V.N)
    out = [rp, ci, kr.pattern_values(orc.mass_matrix(S), rp, ci)]
    if with_stiffness:
        out.append(kr.pattern_values(orc.stiffness_matrix(S), rp, ci))
    return tuple(out), lay


@functools.lru_cache(maxsize=None)
def world():
    from flow_amd import fem
    p1, _ = _pattern(fem.UnitSquareMesh(4, 4), 1, False)
    p2, lay2 = _pattern(fem.UnitSquareMesh(10, 10, 'crossed'), 2, True)
    systems = kr.small_systems(p1, p2)
    pb, _ = _pattern(fem.RectangleMesh(fem.Point(0.0, 0.0), fem.Point(2.0, 1.0),
                                       BIG[0], BIG[1]), 1, False)
    systems['big'] = kr.System(0, pb[0], pb[1], [pb[2]])
    vecs = dict((k, kr.starts(k, S)) for k, S in systems.items())
    # a two-level map over 3 x 3 bins of the dof coordinates
    x = lay2.dof_coords
    agg = (numpy.floor(x[:, 0] * 3 - 1e-9).clip(0) * 3
           + numpy.floor(x[:, 1] * 3 - 1e-9).clip(0)).astype(numpy.int64)
    S = systems['p2']
    P = numpy.zeros((S.N, 9))
    P[numpy.arange(S.N), agg] = 1.0
    Ainv32 = numpy.linalg.inv(P.T.dot(S.A.dot(P))).astype(numpy.float32)
    return systems, vecs, (agg, Ainv32)


def precond(case, weight=1.0):
    systems, _, (agg, Ainv32) = world()
    S = systems[case['system']]
    pre = case['pre']
    if pre == 'none':
        return kr.identity
    if pre == 'jacobi':
        return lambda dtype: kr.jacobi(S.dinv, dtype)
    assert pre == 'two_level'
    return lambda dtype: kr.two_level(S.dinv, agg, Ainv32, dtype, weight)


@functools.lru_cache(maxsize=None)
def measured(cid):
    case = BY_ID[cid]
    systems, vecs, _ = world()
    return kr.Measured(case, systems[case['system']], precond(case),
                       vecs[case['system']])


HOST_CASES = [c for c in kr.CASES + kr.COUNT_CASES
              if c['pre'] in kr.HOST_PRECONDITIONERS]
BY_ID = dict((c['id'], c) for c in HOST_CASES)
assert len(BY_ID) == len(HOST_CASES)


def test_case_ids_are_unique():
    ids = [c['id'] for c in kr.CASES + kr.COUNT_CASES]
    assert len(set(ids)) == len(ids)


@pytest.mark.parametrize('cid', sorted(c['id'] for c in HOST_CASES
                                        if c in kr.CASES))
def test_tolerance_and_conditions(cid):
    case = BY_ID[cid]
    m = measured(cid)
    systems, vecs, _ = world()
    S, v = systems[case['system']], vecs[case['system']]
    print('MEASURED %-44s N %6d K %2d d %.2e tol %.2e'
          % (cid, S.N, m.K, m.d, m.tol))
    assert m.K >= kr.MIN_ITERATES
    for k in range(m.K + 1):
        assert m.ext.norms[k] >= kr.FLOOR * m.ext.norms[0]
    # by construction; and the tolerance is a tolerance
    assert m.d * kr.MARGIN <= m.tol < 1.0e-7
    restart = case['opts'].get('restart')
    if restart is not None and restart < 30:
        assert m.K >= 2 * restart + 1
    if restart == 30 and case in kr.CASES and case['system'] != 'm25':
        assert m.K >= 10          # (the second chunk of eight, with a remainder)
    A, b = S.op(kr.EXT), v['b'].astype(kr.EXT)
    if case['start'] in ('kept', 'dropped'):
        r0 = b - A(v[case['start']].astype(kr.EXT))
        B = precond(case)(kr.EXT)
        if case['start'] == 'kept':
            assert kr.norm(r0) < 0.9 * kr.norm(b)
            assert kr.norm(B(r0)) < 0.9 * kr.norm(B(b))
        else:
            assert kr.norm(r0) > 10.0 * kr.norm(b)
            zero = dict(case, start='zero')
            t0 = kr.reference(zero, S, precond(case), v)
            assert kr.departure(m.ext, t0, m.K) == 0.0
    if case['system'] == 'masked':
        fixed = S.mask == 0
        assert 0.05 < fixed.mean() < 0.09
        assert (v['nonzero'][fixed] == v['b'][fixed]).all()


@pytest.mark.parametrize('case', kr.COUNT_CASES, ids=lambda c: c['id'])
def test_count_conditions(case):
    m = measured(case['id'])
    kstar, rtol, rels = kr.count_target(m.ext, case['solver'])
    print('COUNT %s k* %d rtol %.3e rels %s'
          % (case['id'], kstar, rtol, ' '.join('%.2e' % r for r in rels)))
    tol = kr.count_tolerance(m, kstar)
    print('MEASURED %-44s N %6d k* %d d %.2e tol %.2e'
          % (case['id'], m.ext.xs[0].size, kstar, tol / kr.MARGIN, tol))
    assert 2 <= kstar <= m.K and tol < 1.0e-7
    assert rels[kstar - 1] >= 10.0 * rels[kstar]
    assert min(rels[:kstar]) >= 3.0 * rtol >= 9.0 * rels[kstar]
    if case['solver'] == 'gmres':
        true = float(m.ext.norms[kstar])
        assert abs(float(m.ext.est[kstar]) - true) <= 0.01 * true
        # (no cancellation in the Pythagoras estimate at k*: the driver's
        # "lucky" exit needs a sub-diagonal below 1e-6 of the column)
        assert rels[kstar] > 1.0e-6


# mutant -> the cases it must show in (at least one of them)
MUTANTS = {
    'stale_beta': ['cg-p2-jacobi-zero', 'cg-m25-none-zero'],
    'shift:cg': ['cg-p2-jacobi-zero'],
    'shift:bicgstab': ['bicgstab-block-jacobi-zero'],
    'shift:gmres': ['gmres-block-jacobi-zero-r4'],
    'left:bicgstab': ['bicgstab-block-jacobi-zero', 'bicgstab-p2-jacobi-nonzero'],
    'left:gmres': ['gmres-block-jacobi-zero-r4', 'gmres-p2-jacobi-kept-r30'],
    'half_coarse': ['cg-p2-two_level-zero', 'cg-p2-two_level-nonzero'],
    'drop_h4': ['gmres-block-none-zero-r30-x1', 'gmres-p2-none-zero-r7-x1'],
    'estimated_restart': ['gmres-block-jacobi-zero-r4',
                          'gmres-p2-none-zero-r7-x1'],
    }


@pytest.mark.parametrize('name', sorted(MUTANTS))
def test_mutants_clear_the_tolerance(name):
    systems, vecs, _ = world()
    mutant = name.split(':')[0]
    best = 0.0
    for cid in MUTANTS[name]:
        case = BY_ID[cid]
        m = measured(cid)
        S, v = systems[case['system']], vecs[case['system']]
        if mutant == 'half_coarse':
            t = kr.reference(case, S, precond(case, weight=0.5), v)
        else:
            t = kr.reference(case, S, precond(case), v, mutant=mutant)
        ratio = kr.departure(t, m.ext, m.K) / m.tol
        print('MUTANT %-18s %-34s %.3g tolerances' % (name, cid, ratio))
        best = max(best, ratio)
    assert best >= 1000.0


def test_first_departure_names_the_iterate():
    '''A stale beta leaves x_0, x_1 and x_2 alone (beta first enters p_1,
    the stale one is 0 there: x_2 moves) -- the comparison names the first
    iterate that differs.'''
    systems, vecs, _ = world()
    case = BY_ID['cg-p2-jacobi-zero']
    m = measured(case['id'])
    t = kr.reference(case, systems['p2'], precond(case), vecs['p2'],
                     mutant='stale_beta')
    bad = [k for k in range(m.K + 1) if kr.rel(t.xs[k], m.ext.xs[k]) > m.tol]
    assert bad[0] == 2 and bad == list(range(2, m.K + 1))
