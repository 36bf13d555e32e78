# -*- coding: utf-8 -*-
'''
Forms of test and trial functions on a Taylor-Hood space, host side
(flow_amd/fem/forms.py, mixed_arguments; space.RectLayout): the switch, the
3 x 3 block tables, symmetry detection, the refusals and the rectangular
pattern with its contribution maps.  No GPU.
'''
import numpy
import pytest
import scipy.sparse as sp

from flow_amd import fem
from flow_amd.fem import (
    TestFunction, TrialFunction, dx, inner, grad, div, dot, forms, space,
    )


def _space(mesh, kv=2, kp=1):
    return fem.FunctionSpace(
        mesh, fem.VectorElement('Lagrange', 'triangle', kv)
        * fem.FiniteElement('Lagrange', 'triangle', kp))


@pytest.fixture
def on():
    with fem.mixed_arguments(True), fem.vector_arguments(True):
        yield


def _reference_form(WP, sign=-1.0):
    (u, p) = fem.TrialFunctions(WP)
    (v, q) = fem.TestFunctions(WP)
    mu = fem.Constant(0.7)
    return mu * inner(grad(u), grad(v)) * dx - p * div(v) * dx \
        + sign * q * div(u) * dx


def test_switch_off_everything_raises_as_before():
    WP = _space(fem.UnitSquareMesh(3, 2))
    assert not fem.mixed_arguments.enabled
    for fn in (fem.TestFunctions, fem.TrialFunctions, TestFunction,
               TrialFunction):
        with pytest.raises(NotImplementedError,
                           match='only scalar P1 / P2 spaces carry arguments'):
            fn(WP)
    with pytest.raises(AssertionError):
        fem.Function(WP)
    with fem.mixed_arguments(True):
        assert fem.mixed_arguments.enabled
        with pytest.raises(NotImplementedError, match='vector_arguments'):
            fem.TestFunctions(WP)
    assert not fem.mixed_arguments.enabled


def test_block_tables_of_the_reference_form(on):
    WP = _space(fem.UnitSquareMesh(3, 2))
    (u, p), (v, q) = fem.TrialFunctions(WP), fem.TestFunctions(WP)
    assert v.shape == (2,) and q.shape == () and u.shape == (2,)
    mu = fem.Constant(0.7)
    one = (mu * inner(grad(u), grad(v)) - p * div(v) - q * div(u)) * dx
    rank, table = one.argument_table()
    assert rank == 2 and isinstance(table, forms.MixedTable)
    present = {(r, s) for r in range(3) for s in range(3)
               if table[r][s] is not None}
    assert present == {(0, 0), (1, 1), (0, 2), (1, 2), (2, 0), (2, 1)}
    assert forms.is_symmetric_table(table)
    # the corner is the BlockTable of the same terms on the velocity space
    W = WP.sub(0)
    uw, vw = TrialFunction(W), TestFunction(W)
    _, want = (mu * inner(grad(uw), grad(vw)) * dx).argument_table()
    corner = table.velocity()
    assert type(corner) is forms.BlockTable and corner == want
    # rank 1
    rank, t1 = (inner(fem.Constant((1.0, 2.0)), v) * dx
                + 3.0 * q * dx).terms()[0][1].argument_table()
    assert rank == 1 and t1[0] is not None and t1[1] is not None \
        and t1[2] is None


def test_symmetry_of_the_sum_of_parts(on):
    WP = _space(fem.UnitSquareMesh(3, 2))
    assert forms.is_symmetric_form(_reference_form(WP))
    assert not forms.is_symmetric_form(_reference_form(WP, +1.0))
    flipped = _reference_form(WP, +1.0)
    (u, p), (v, q) = fem.TrialFunctions(WP), fem.TestFunctions(WP)
    mu = fem.Constant(0.7)
    whole = (mu * inner(grad(u), grad(v)) - p * div(v) + q * div(u)) * dx
    assert not forms.is_symmetric_table(whole.argument_table()[1])
    assert flipped.rank == 2


def test_nonlinear_and_mixed_rank_forms_are_refused(on):
    WP = _space(fem.UnitSquareMesh(3, 2))
    (u, p), (v, q) = fem.TrialFunctions(WP), fem.TestFunctions(WP)
    with pytest.raises(ValueError, match='not linear'):
        (p * p * q * dx).argument_table()
    with pytest.raises(ValueError, match='not linear'):
        (q / p * dx).argument_table()
    with pytest.raises(ValueError, match='differ in rank'):
        ((p * q + q) * dx).argument_table()
    with pytest.raises(ValueError, match='without the test function'):
        (p * dx).argument_table()


def test_refused_combinations(on):
    mesh = fem.UnitSquareMesh(3, 2)
    WP = _space(mesh)
    (u, p), (v, q) = fem.TrialFunctions(WP), fem.TestFunctions(WP)
    P = fem.FunctionSpace(mesh, 'CG', 1)
    with pytest.raises(NotImplementedError, match='mixed space together'):
        (TrialFunction(P) * q * dx).arguments()
    W = fem.VectorFunctionSpace(mesh, 'CG', 2)
    with pytest.raises(NotImplementedError, match='mixed space together'):
        (dot(TrialFunction(W), v) * dx).arguments()
    # (derivative() and solve(F == 0) need a Function(WP), so a device:
    # tests/test_mixed_forms_gpu.py)
    for fn in (fem.TestFunctions, fem.TrialFunctions):
        for V in (P, W):
            with pytest.raises(NotImplementedError,
                               match='takes a mixed .* space and returns a pair'):
                fn(V)
    other = fem.FunctionSpace(
        mesh, fem.VectorElement('Lagrange', 'triangle', 2)
        * fem.VectorElement('Lagrange', 'triangle', 1))
    with pytest.raises(NotImplementedError, match='Taylor-Hood'):
        fem.TestFunctions(other)
    with pytest.raises(NotImplementedError, match='take the pair'):
        TestFunction(WP)
    with fem.interior_facets(True):
        with pytest.raises(NotImplementedError,
                           match='test and trial functions under dS'):
            fem.jump(p) * fem.jump(q) * fem.dS
        with pytest.raises(NotImplementedError,
                           match='test and trial functions under dS'):
            fem.avg(p) * fem.jump(v[0]) * fem.dS
    with pytest.raises(TypeError, match='split takes a Function'):
        fem.split(v)


def test_eigenmodes_and_strips_are_refused(on, monkeypatch):
    WP = _space(fem.UnitSquareMesh(3, 2))
    a = _reference_form(WP)
    (u, p), (v, q) = fem.TrialFunctions(WP), fem.TestFunctions(WP)
    with pytest.raises(NotImplementedError,
                       match='Eigenmodes of forms on a mixed space'):
        fem.Eigenmodes(a)
    with fem.vector_eigenmodes(True):
        with pytest.raises(NotImplementedError,
                           match='Eigenmodes of forms on a mixed space'):
            fem.Eigenmodes(a, m=dot(u, v) * dx + p * q * dx)
    from flow_amd import parallel
    monkeypatch.setattr(parallel, 'active', lambda: True)
    L = inner(fem.Constant((1.0, 0.0)), v) * dx
    with pytest.raises(NotImplementedError, match='assemble on strips'):
        fem.assemble(a)
    with pytest.raises(NotImplementedError, match='assemble on strips'):
        fem.assemble(L)
    with pytest.raises(NotImplementedError,
                       match='assemble_system on strips'):
        fem.assemble_system(a, L, [])
    with pytest.raises(NotImplementedError, match='solve on strips'):
        fem.solve(a == L, None, [])


def _check_rect(mesh, dr, dc):
    R = space.RectLayout(mesh, dr, dc)
    rows, cols = space.scalar_layout(mesh, dr), space.scalar_layout(mesh, dc)
    nc = mesh.num_cells()
    nlr, nlc = rows.nloc, cols.nloc
    i = numpy.repeat(rows.cell_dofs, nlc, axis=1).ravel()
    j = numpy.tile(cols.cell_dofs, (1, nlr)).ravel()
    S = sp.coo_matrix((numpy.ones(len(i)), (i, j)),
                      shape=(rows.N, cols.N)).tocsr()
    S.sort_indices()
    assert R.shape == S.shape and R.nnz == S.nnz
    assert numpy.array_equal(R.rowptr, S.indptr)
    assert numpy.array_equal(R.cols, S.indices)
    # every (cell, i, j) exactly once; sources of a target ascend by cell and
    # land on the target's (row, col)
    assert numpy.array_equal(numpy.sort(R.csrc), numpy.arange(nlr * nlc * nc))
    assert R.cptr[0] == 0 and R.cptr[-1] == nlr * nlc * nc
    assert (numpy.diff(R.cptr) >= 1).all()
    cell, ij = R.csrc % nc, R.csrc // nc
    target = numpy.repeat(numpy.arange(R.nnz), numpy.diff(R.cptr))
    trow = numpy.repeat(numpy.arange(rows.N), numpy.diff(R.rowptr))[target]
    assert numpy.array_equal(rows.cell_dofs[cell, ij // nlc], trow)
    assert numpy.array_equal(cols.cell_dofs[cell, ij % nlc], R.cols[target])
    same = target[1:] == target[:-1]
    assert (cell[1:][same] > cell[:-1][same]).all()
    # the list maps: every scratch entry once, targets sorted and unique
    for targets, ptr, src in (R.facet_map_host(), R.cell_map_host()):
        assert numpy.array_equal(numpy.sort(src), numpy.arange(len(src)))
        assert (numpy.diff(targets) > 0).all() and ptr[-1] == len(src)
    targets, ptr, src = R.cell_map_host()
    assert numpy.array_equal(targets, numpy.arange(R.nnz))
    assert numpy.array_equal(ptr, R.cptr) and numpy.array_equal(src, R.csrc)
    assert space.rect_layout(mesh, dr, dc) is space.rect_layout(mesh, dr, dc)
    # the mirror image of every entry in the transposed pattern
    T = space.RectLayout(mesh, dc, dr)
    perm = space.transpose_permutation(R.rowptr, R.cols, T.rowptr, T.cols)
    back = space.transpose_permutation(T.rowptr, T.cols, R.rowptr, R.cols)
    tcol = numpy.repeat(numpy.arange(cols.N), numpy.diff(T.rowptr))
    rrow = numpy.repeat(numpy.arange(rows.N), numpy.diff(R.rowptr))
    assert numpy.array_equal(T.cols[perm], rrow)
    assert numpy.array_equal(tcol[perm], R.cols)
    assert numpy.array_equal(back[perm], numpy.arange(R.nnz))


@pytest.mark.parametrize('degrees', [(2, 1), (1, 2)])
def test_rect_layout(degrees):
    _check_rect(fem.UnitSquareMesh(3, 2), *degrees)
    _check_rect(fem.karman_channel(60, 14, fitted=True), *degrees)
