# -*- coding: utf-8 -*-
'''
Host logic of the non-symmetric mixed solve (flow_amd/fem/mixed.py,
fem.mixed_gmres): the row tiles of flow_mixed_apply, the switch and the
dispatch predicate of solve, and the signed approximate Schur diagonal restated
in numpy.  No GPU.
'''
import numpy
import pytest
import scipy.sparse as sp

from flow_amd import fem, _hip
from flow_amd.fem import forms, mixed
from flow_amd.fem.space import csr_stream_rowblocks, transpose_permutation


def _meshes():
    return [fem.UnitSquareMesh(12, 9), fem.karman_channel(60, 14, fitted=True)]


PAIRS = [(2, 1), (1, 1)]


def test_tiles_cover_rows_once_within_both_caps():
    cap = mixed._tile_cap()
    assert cap == _hip.SPMV_NNZ_PER_BLOCK
    several = 0
    for mesh in _meshes():
        for kv, kp in PAIRS:
            for R in (fem.rect_layout(mesh, kv, kp),
                      fem.rect_layout(mesh, kp, kv)):
                tiles = mixed.fused_tiles(R)
                assert tiles is mixed.fused_tiles(R)      # held on the layout
                n = R.rows.N
                assert tiles.dtype == numpy.int32
                assert tiles[0] == 0 and tiles[-1] == n
                rows = numpy.diff(tiles)
                assert (rows > 0).all() and rows.max() <= 256
                for rp in (R.rows.pattern('rowptr'), R.rowptr):
                    rp = numpy.asarray(rp, dtype=numpy.int64)
                    assert len(rp) == n + 1
                    assert numpy.diff(rp[tiles]).max() <= cap
                several += len(tiles) - 1 > 1
                # a tile ends where one more row would break a limit
                sq = numpy.asarray(R.rows.pattern('rowptr'), dtype=numpy.int64)
                re = numpy.asarray(R.rowptr, dtype=numpy.int64)
                for t in range(len(tiles) - 2):
                    r0, r1 = tiles[t], tiles[t + 1]
                    assert r1 - r0 == 256 or sq[r1 + 1] - sq[r0] > cap \
                        or re[r1 + 1] - re[r0] > cap
    assert several >= 4
    # P2 on the unit square: tile boundaries at odd nonzero offsets
    R = fem.rect_layout(fem.UnitSquareMesh(12, 9), 2, 1)
    assert (R.rows.pattern('rowptr')[mixed.fused_tiles(R)] & 1).any()


def test_row_longer_than_the_cap_is_refused():
    ok = numpy.arange(0, 50, 5)
    long_row = numpy.array([0, 3, 3 + _hip.SPMV_NNZ_PER_BLOCK + 1, 1100, 1103,
                            1106, 1109, 1112, 1115, 1118])
    assert len(ok) == len(long_row)
    csr_stream_rowblocks([ok, ok], nnz_per_block=_hip.SPMV_NNZ_PER_BLOCK)
    for pair in ([ok, long_row], [long_row, ok]):
        with pytest.raises(AssertionError,
                           match='row longer than the CSR-stream LDS tile'):
            csr_stream_rowblocks(pair,
                                 nnz_per_block=_hip.SPMV_NNZ_PER_BLOCK)


def test_switch_and_dispatch_predicate():
    assert issubclass(fem.mixed_gmres, forms._Switch)
    assert fem.mixed_gmres is forms.mixed_gmres
    assert fem.mixed_gmres.enabled is False
    assert mixed.solver_route(False, {}) == 'refuse'
    assert mixed.solver_route(True, {}) == 'minres'
    assert mixed.solver_route(True, {'linear_solver': 'gmres'}) == 'minres'
    assert mixed.solver_route(False, {'symmetric': False}) == 'refuse'
    with fem.mixed_gmres(True) as sw:
        assert sw.previous is False and fem.mixed_gmres.enabled is True
        # it implies no other switch
        assert not forms.mixed_arguments.enabled
        assert not forms.vector_arguments.enabled
        assert mixed.solver_route(False, {}) == 'fgmres'
        assert mixed.solver_route(True, {}) == 'minres'
        assert mixed.solver_route(True, {'linear_solver': 'gmres'}) == 'fgmres'
        with fem.mixed_gmres(False):
            assert mixed.solver_route(False, {}) == 'refuse'
        assert fem.mixed_gmres.enabled is True
    assert fem.mixed_gmres.enabled is False
    assert mixed.solver_route(False, {}) == 'refuse'


def _schur_numpy(pp_diag, pu, up, dinv, perms):
    '''mixed._signed_schur_diagonal entry by entry: the plane of pu[s] times
    the mirror entries of up[s], applied to dinv_s, subtracted from diag(pp);
    zero rows 1.'''
    d = pp_diag.copy()
    for s in range(2):
        both = sp.csr_matrix((pu[s].data * up[s].data[perms[s]],
                              pu[s].indices, pu[s].indptr), shape=pu[s].shape)
        d -= both @ dinv[s]
    return numpy.where(d != 0.0, d, 1.0)


def test_signed_schur_diagonal_formula_mirror_and_sign():
    rng = numpy.random.RandomState(11)
    nv, npr = 23, 9
    pat = sp.random(npr, nv, 0.3, random_state=rng, format='csr')
    pat.data[:] = 1.0
    pat = sp.csr_matrix(pat)
    pat.sort_indices()
    patT = sp.csr_matrix(pat.T)
    patT.sort_indices()
    perm = transpose_permutation(pat.indptr, pat.indices, patT.indptr,
                                 patT.indices)
    # the permutation reaches the mirror entry
    marks = sp.csr_matrix((numpy.arange(1.0, patT.nnz + 1), patT.indices,
                           patT.indptr), shape=patT.shape)
    dense = marks.toarray()
    rows = numpy.repeat(numpy.arange(npr), numpy.diff(pat.indptr))
    assert numpy.array_equal(marks.data[perm], dense[pat.indices, rows])

    def plane(P):
        return sp.csr_matrix((rng.standard_normal(P.nnz), P.indices,
                              P.indptr), shape=P.shape)

    up = [plane(patT), plane(patT)]          # independent of pu: Oseen-like
    pu = [plane(pat), plane(pat)]
    dinv = [1.0 / rng.uniform(0.5, 2.0, nv) for _ in range(2)]
    pp_diag = rng.standard_normal(npr)
    got = _schur_numpy(pp_diag, pu, up, dinv, [perm, perm])
    want = pp_diag - sum(
        (pu[s] @ sp.diags(dinv[s]) @ up[s]).diagonal() for s in range(2))
    want = numpy.where(want != 0.0, want, 1.0)
    assert numpy.abs(got - want).max() <= 1e-14 * numpy.abs(want).max()
    # pu = +up^T (the symmetric form, written with -q*div(u)): a negative
    # diagonal, -B F^-1 B^T; pu = -up^T (+q*div(u)): the same, positive
    zero = numpy.zeros(npr)
    minus = [sp.csr_matrix(-B.T) for B in up]
    plus = [sp.csr_matrix(B.T) for B in up]
    for P in minus + plus:
        P.sort_indices()
        assert numpy.array_equal(P.indices, pat.indices)
    dm = _schur_numpy(zero, minus, up, dinv, [perm, perm])
    dp = _schur_numpy(zero, plus, up, dinv, [perm, perm])
    empty = numpy.diff(pat.indptr) == 0
    assert (dm[~empty] > 0.0).all() and (dp[~empty] < 0.0).all()
    assert numpy.array_equal(dm[~empty], -dp[~empty])
    assert (dm[empty] == 1.0).all() and (dp[empty] == 1.0).all()
    exact = sum((up[s].T.multiply(up[s].T) @ dinv[s]) for s in range(2))
    exact = numpy.asarray(exact).ravel()
    assert numpy.abs(dm[~empty] - exact[~empty]).max() <= 1e-14 * exact.max()
