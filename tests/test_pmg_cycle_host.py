# -*- coding: utf-8 -*-
'''
The launch-by-launch check of the p-multigrid cycle (tests/
test_pmg_cycle_gpu.py) without a GPU: the model (tests/pmg_cycle_reference.py)
is the algorithm -- its float64 composition equals the textbook cycle of
tests/test_pmg.py for every (pre, post, coarse_steps) of the grid --, the
comparator accepts the same launches evaluated in fp32 through the work-buffer
layout of pmg_apply, and it rejects that stand-in with one seeded defect each
(pmg_cycle_reference.MUTATIONS).

What the comparator cannot see: nothing of the list in MUTATIONS.  Two defects
need their own inputs to be material and get them: 'post_continues' changes
nothing while pre = 1 (the pre-smoothing never calls Cheb::next then; the grid
holds pre = 2 and 3 with post >= 2), and 'bc_stride' needs a dof that is a
Dirichlet dof in one component only (Problem provides one per component).
'''
import functools
from types import SimpleNamespace

import numpy
import pytest
import scipy.sparse as sp

import pmg_cycle_reference as cyc
from test_pmg import _cycle

MESHES = ('rect', 'karman')


@functools.lru_cache(maxsize=None)
def _problem(mesh, variant='vector', g=0):
    if variant == 'block':
        return cyc.Problem(mesh, block=(g, 3))
    return cyc.Problem(mesh, one_plane=variant == 'one_plane',
                       scalar=variant == 'scalar')


def test_the_inputs_hold_what_they_advertise():
    rect, karman = _problem('rect'), _problem('karman')
    assert (rect.n, rect.n1) == (165, 48) and (karman.n, karman.n1) == (1272, 340)
    lens = numpy.concatenate([rect.list_lengths(), karman.list_lengths()])
    # all three paths of pmg_restrict_kernel
    assert (lens < cyc.K_AHEAD).any() and (lens == cyc.K_AHEAD).any() \
        and (lens > cyc.K_AHEAD).any()
    for p in (rect, karman):
        lay2 = p.lay2
        kind = numpy.zeros(p.n, dtype=int)
        kind[lay2.edge_dofs] = 1
        for a in (0, 1):
            rows = numpy.nonzero(p.bc[:, a])[0]
            assert set(kind[rows]) == {0, 1}
        v, e = p.single
        assert tuple(p.bc[v]) == (1, 0) and tuple(p.bc[e]) == (0, 1)
        assert p.bcc.sum() > 0 and (p.bcc[:, 0] != p.bcc[:, 1]).any()
        # identity rows, distinct planes, garbage in the planes to ignore
        assert not numpy.array_equal(p.planes[0], p.planes[3])
        assert abs(p.planes[1]).min() > 0.0 and abs(p.planes[2]).max() > 1e5
        for L, bc in ((p.fine, p.bc), (p.coarse, p.bcc)):
            w = L.w.astype(numpy.float64)
            off = numpy.ones(L.nnz, dtype=bool)
            off[L.diag_idx] = False
            assert (w[L.diag_idx] == 1.0).all()
            for a in (0, 1):
                cnt = numpy.bincount(L.row_of, weights=(off & (w[:, a] != 0)),
                                     minlength=L.n)
                assert numpy.array_equal(cnt == 0, bc[:, a] != 0)
            assert 0.0 < L.lo < L.hi
    # the one-plane level finds the Dirichlet dofs as its identity rows
    one = _problem('rect', 'one_plane')
    assert numpy.array_equal(one.fine.idrows, one.bc)
    assert numpy.array_equal(one.coarse.idrows, one.bcc)
    # the blocks of the strips read the dummy coarse row (an edge dof belongs
    # to its lower vertex: all but the last block have partners outside)
    for g in range(3):
        b = _problem('karman', 'block', g)
        assert b.ends.max() <= b.n1 and (b.ends == b.n1).any() == (g < 2)
        assert not b.keep[0].all() and not b.keep[1].all()
        assert (b.fine.w[~b.keep[0]] == 0).all()


@pytest.mark.parametrize('mesh', MESHES)
def test_the_model_is_the_textbook_cycle(mesh):
    '''cycle_f64 without any fp32 in it against _cycle / _cheb of
    tests/test_pmg.py on A = D W16: to 1e-12 for every configuration.'''
    p = _problem(mesh)
    n, n1 = p.n, p.n1
    rows = numpy.repeat(numpy.arange(n), 2)
    P = sp.csr_matrix((numpy.full(2 * n, 0.5), (rows, p.ends.ravel())),
                      shape=(n, n1))
    mats = []
    for L in (p.fine, p.coarse):
        D = L.diag.astype(numpy.float64)
        mats.append([sp.diags(D[:, a]).dot(sp.csr_matrix(
            (L.w[:, a].astype(numpy.float64), L.cols, L.rp),
            shape=(L.n, L.n))).tocsr() for a in (0, 1)])
    r = p.rhs(0)
    for cfg in cyc.GRID:
        pre = SimpleNamespace(
            fine=SimpleNamespace(struct=SimpleNamespace(
                lam_min=p.fine.lo, lam_max=p.fine.hi)),
            coarse=SimpleNamespace(struct=SimpleNamespace(
                lam_min=p.coarse.lo, lam_max=p.coarse.hi)),
            struct=SimpleNamespace(pre=cfg[0], post=cfg[1],
                                   coarse_steps=cfg[2]))
        z, _bound = cyc.cycle_f64(cfg, p, r, exact=True)
        for a in (0, 1):
            want = _cycle(pre, mats[0][a], mats[1][a], P, p.bc[:, a] != 0,
                          p.bcc[:, a] != 0, r[a * n:(a + 1) * n])
            assert abs(z[:, a] - want).max() <= 1e-12 * abs(want).max(), cfg


def _accept(p, configs, tag):
    worst = {}
    for trial in (0, 1):
        r = p.rhs(trial)
        runs = cyc.standin_runs(p, r, configs)
        for kind, ratio in cyc.compare(p, r, runs, '%s trial %d' %
                                       (tag, trial)).items():
            worst[kind] = max(ratio, worst.get(kind, 0.0))
    print('WORST host stand-in %s: %s' % (tag, ' '.join(
        '%s %.3g' % (k, worst[k]) for k in cyc.KINDS if k in worst)))
    assert max(worst.values()) <= 1.0
    return worst


@pytest.mark.parametrize('mesh', MESHES)
def test_comparator_accepts_the_cycle_in_fp32(mesh):
    worst = _accept(_problem(mesh), cyc.GRID, 'host ' + mesh)
    assert set(worst) == set(cyc.KINDS)       # every launch kind was compared


@pytest.mark.parametrize('variant', ['one_plane', 'scalar', 'block'])
def test_comparator_accepts_the_variants_in_fp32(variant):
    if variant == 'block':
        for g in range(3):
            _accept(_problem('karman', 'block', g), cyc.family(2, 2, 3),
                    'host block %d' % g)
        return
    configs = cyc.family(2, 3, 3) + ((1, 1, 1),) * (variant == 'scalar')
    for mesh in MESHES:
        _accept(_problem(mesh, variant), configs, 'host %s %s' % (variant, mesh))


def test_scalar_mode_ignores_what_lies_behind_r():
    p = _problem('rect', 'scalar')
    r = p.rhs(0)
    assert numpy.isnan(r[p.n:]).all()
    run = cyc.standin_runs(p, r, [(1, 1, 1)])[(1, 1, 1)]
    assert numpy.isfinite(run['z']).all() and run['z'].shape == (p.n, 1)


# -- every seeded defect is rejected -------------------------------------------------
WHERE = {'scalar_z_tail': ('rect', 'scalar'), 'dummy_nonzero': ('karman', 'block'),
         'no_tail': ('rect', 'vector')}


@pytest.mark.parametrize('mutation', cyc.MUTATIONS)
def test_comparator_rejects(mutation):
    mesh, variant = WHERE.get(mutation, ('karman', 'vector'))
    p = _problem(mesh, variant)
    configs = {'vector': cyc.GRID, 'scalar': cyc.family(2, 3, 3),
               'block': cyc.family(2, 2, 3)}[variant]
    r = p.rhs(0)
    clean = cyc.standin_runs(p, r, configs)
    cyc.compare(p, r, clean, 'clean')
    bad = cyc.standin_runs(p, r, configs, mut=[mutation])
    changed = [cfg for cfg in configs
               if any(not numpy.array_equal(clean[cfg][k], bad[cfg][k])
                      for k in clean[cfg])]
    assert changed, 'the defect changes nothing'
    with pytest.raises(AssertionError, match='times its bound'):
        cyc.compare(p, r, bad, mutation)
