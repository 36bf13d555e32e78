# -*- coding: utf-8 -*-
'''
Test and trial functions under ds on the host (flow_amd/fem/forms.py,
ops.facet_map_host): ranks and tables of Neumann, Robin and Nitsche terms,
lhs / rhs / system of a Robin integrand, derivative of ds parts, every refusal
that needs no device, the invariants of the facet contribution map, and the
numpy evaluator of tests/facet_argument_reference.py against closed forms.
No GPU.
'''
import numpy
import pytest

from flow_amd import fem
from flow_amd.fem import (
    TestFunction, TrialFunction, dx, ds, dot, grad, lhs, rhs, system, forms,
    derivative, Measure, MeshFunction, FacetNormal, conditional, gt,
    SpatialCoordinate, CellDiameter,
    )
from flow_amd.fem import ops

import facet_argument_reference as faref

ONE = ('num', 1.0)


@pytest.fixture(autouse=True)
def _facet_arguments_on():
    '''Arguments under ds are off by default: on for these tests only.'''
    with fem.facet_arguments(True):
        yield


def test_off_by_default():
    '''The switch: off, the refusals are what they were; on, it reports the
    setting it replaced and a `with` block restores it.'''
    mesh, V1, _ = _spaces()
    u, v = TrialFunction(V1), TestFunction(V1)
    w = fem.Function(V1)
    assert fem.facet_arguments.enabled          # (the fixture of this file)
    with fem.facet_arguments(False) as off:
        assert off.previous is True and not fem.facet_arguments.enabled
        with pytest.raises(NotImplementedError, match='contribution map'):
            v * ds
        with pytest.raises(NotImplementedError, match='under ds'):
            u * v * ds(mesh)
        with pytest.raises(NotImplementedError, match='contribution map'):
            derivative(w**2 * ds, w)
        # functionals over ds never needed the switch
        assert (w * ds).rank == 0
    assert fem.facet_arguments.enabled
    assert (v * ds).rank == 1


def _spaces(nx=3, ny=2):
    mesh = fem.UnitSquareMesh(nx, ny)
    return (mesh, fem.FunctionSpace(mesh, 'CG', 1),
            fem.FunctionSpace(mesh, 'CG', 2))


class _Left(fem.SubDomain):
    def inside(self, x, on_boundary):
        return on_boundary & (x[0] < 1e-12)


def _marked(mesh):
    m = MeshFunction('size_t', mesh, 1, 0)
    _Left().mark(m, 2)
    return m, Measure('ds', domain=mesh, subdomain_data=m)


def test_measure_accepts_arguments_and_ranks():
    mesh, V1, V2 = _spaces()
    m, dsm = _marked(mesh)
    n = FacetNormal(mesh)
    for V in (V1, V2):
        u, v = TrialFunction(V), TestFunction(V)
        L = fem.Constant(2.0) * v * dsm(2)
        assert L.integral_type == 'exterior_facet' and L.rank == 1
        assert L.subdomain_id == 2 and L.subdomain_data is m
        rank, tab = L.argument_table()
        assert rank == 1 and tab[0][0] == 'const' and tab[1:] == [None, None]
        a = u * v * ds
        assert a.integral_type == 'exterior_facet' and a.rank == 2
        assert a.arguments() == {0: V, 1: V}
        rank, tab = a.argument_table()
        assert rank == 2 and tab[0][0] == ONE
        assert sum(t is not None for row in tab for t in row) == 1
        assert forms.is_symmetric_table(tab)
        # the normal stays legal, and the off-diagonal table is not symmetric
        nit = -dot(grad(u), n) * v * ds(mesh)
        rank, tab = nit.argument_table()
        assert rank == 2
        assert tab[0][1] == ('neg', ('n', 0)) and tab[0][2] == ('neg', ('n', 1))
        assert not forms.is_symmetric_table(tab)
        sym = (-dot(grad(u), n) * v - u * dot(grad(v), n)) * ds(mesh)
        assert forms.is_symmetric_table(sym.argument_table()[1])
        # sums of dx and ds parts
        s = dot(grad(u), grad(v)) * dx + 3.0 * u * v * dsm(2)
        assert s.rank == 2 and [p.integral_type for _, p in s.terms()] == [
            'cell', 'exterior_facet']
        # the coefficient tables compile with the normal in them
        prog, = forms.argument_programs(tab, 2, facet=True)
        assert prog.nout == 9 and forms.OPS['normal'] in [c[0] for c in prog.code]
        with pytest.raises(ValueError, match='FacetNormal'):
            forms.argument_programs(tab, 2)


def test_robin_integrand_splits():
    mesh, V1, _ = _spaces()
    u, v = TrialFunction(V1), TestFunction(V1)
    h, uinf = fem.Constant(3.0), fem.Constant(0.5)
    m, dsm = _marked(mesh)
    F = dot(grad(u), grad(v)) * dx + h * (u - uinf) * v * dsm(2)
    a, L = system(F)
    assert [p.integral_type for _, p in a.terms()] == ['cell',
                                                       'exterior_facet']
    pa = a.terms()[1][1]
    assert pa.rank == 2 and pa.subdomain_id == 2 and pa.subdomain_data is m
    assert pa.argument_table()[1][0][0] == ('const', h, 0)
    (sign, pl), = L.terms()
    assert sign == -1.0 and pl.rank == 1
    assert pl.integral_type == 'exterior_facet' and pl.subdomain_id == 2
    # h * (-uinf) v, negated by rhs: + h uinf v
    assert pl.argument_table()[1] == [
        ('mul', ('const', h, 0), ('neg', ('const', uinf, 0))), None, None]
    assert lhs(F).rank == 2 and rhs(F).rank == 1
    # unsplit it stays the ValueError of dx parts
    with pytest.raises(ValueError, match='differ in rank'):
        (h * (u - uinf) * v * ds).argument_table()


def test_derivative_of_ds_parts():
    mesh, V1, V2 = _spaces()
    m, dsm = _marked(mesh)
    for V in (V1, V2):
        u = fem.Function(V)
        v, du = TestFunction(V), TrialFunction(V)
        U = ('field', u, 0, 0)
        # a rank-0 ds functional gives a rank-1 ds form
        E = u**2 * dsm(2, degree=5)
        dE = derivative(E, u)
        assert dE.rank == 1 and dE.integral_type == 'exterior_facet'
        assert dE.subdomain_id == 2 and dE.subdomain_data is m
        assert dE.metadata == {'quadrature_degree': 5}
        assert dE.derived_from is E
        assert dE.argument_table()[1] == [('mul', ('num', 2.0), U), None,
                                          None]
        # a rank-1 ds residual part gives a rank-2 ds part; the sign is kept
        eps = fem.Constant(0.3)
        F = dot(grad(u), grad(v)) * dx - eps * u**4 * v * dsm(2)
        J = derivative(F, u)
        (s0, j0), (s1, j1) = J.terms()
        assert (s0, j0.integral_type) == (1.0, 'cell')
        assert (s1, j1.integral_type) == (-1.0, 'exterior_facet')
        assert j1.rank == 2 and j1.subdomain_id == 2 \
            and j1.subdomain_data is m
        rank, tab = j1.argument_table()
        assert forms.is_symmetric_table(tab)
        assert tab[0][0] == ('mul', ('const', eps, 0),
                             ('mul', ('num', 4.0), ('powi', U, 3)))
        assert derivative(F, u, du).rank == 2
        # twice on an energy over ds
        assert derivative(derivative(u**3 * ds, u), u).rank == 2
        # Newton's jobs: the dx parts fuse, the ds parts never do
        jobs = ops.newton_jobs(J, F)
        assert [j[0] for j in jobs] == ['newton', 'facet_matrix',
                                        'facet_vector']
        assert jobs[1][6] is j1 and jobs[2][6] is F.terms()[1][1]
        assert [j[0] for j in ops.newton_jobs(J, F, fuse=False)] == [
            'matrix', 'facet_matrix', 'vector', 'facet_vector']


def test_refusals(monkeypatch):
    from flow_amd import parallel
    mesh, V1, V2 = _spaces()
    u, v = TrialFunction(V1), TestFunction(V1)
    # the vertex rule on a ds part with arguments
    with pytest.raises(ValueError, match='vertex'):
        u * v * ds(metadata={'quadrature_rule': 'vertex'})
    with pytest.raises(ValueError, match='vertex'):
        ops._part_rule(u * v * ds, {'quadrature_rule': 'vertex'})
    # (a functional does not read the key, as before)
    assert (fem.Constant(1.0) * ds(mesh, metadata={
        'quadrature_rule': 'vertex'})).rank == 0
    # interior facets
    with pytest.raises(NotImplementedError, match='dS'):
        u * v * fem.dS
    # arguments on vector or mixed spaces
    W = fem.VectorFunctionSpace(mesh, 'CG', 2)
    with pytest.raises(NotImplementedError, match='vector'):
        TestFunction(W) * ds
    with pytest.raises(NotImplementedError, match='mixed'):
        TestFunction(fem.MixedFunctionSpace(
            mesh, fem.VectorElement('Lagrange', 'triangle', 2)
            * fem.FiniteElement('Lagrange', 'triangle', 1)))
    # not linear
    with pytest.raises(ValueError, match='not linear'):
        (u * u * v * ds).argument_table()
    # ds(k) without markers
    with pytest.raises(ValueError, match='needs markers'):
        ops.facet_map(mesh, V1.layout, 1, None, 3)
    # strips
    monkeypatch.setattr(parallel, 'active', lambda: True)
    for form in (u * v * ds, v * ds(mesh)):
        with pytest.raises(NotImplementedError, match='on strips'):
            fem.assemble(form)


def _scratch_index(rank, nl, nf, k, i, j=0):
    return (i * nl + j) * nf + k if rank == 2 else i * nf + k


@pytest.mark.parametrize('degree', [1, 2])
def test_map_invariants(degree):
    mesh = fem.UnitSquareMesh(4, 3)
    V = fem.FunctionSpace(mesh, 'CG', degree)
    lay, nl, N = V.layout, V.layout.nloc, V.N
    m, _ = _marked(mesh)
    rowptr, cols = lay.pattern('rowptr'), lay.pattern('cols')
    full = {}
    for sel_args in ((None, 'everywhere'), (m, 2), (m, 99)):
        sel = ops._facet_selection(mesh, *sel_args)
        cells = mesh.bfacet_cell[sel]
        nf = len(sel)
        for rank in (1, 2):
            targets, ptr, src = ops.facet_map_host(mesh, lay, rank, *sel_args)
            assert targets.dtype == ptr.dtype == src.dtype == numpy.int32
            if sel_args[1] == 99:
                # an empty selection yields an empty map
                assert nf == 0 and len(targets) == 0 and len(src) == 0
                assert list(ptr) == [0]
                continue
            # every (facet, i, j) of the selection appears exactly once
            assert sorted(src) == list(range(nf * nl**rank))
            # targets: unique, sorted, inside the pattern
            assert (numpy.diff(targets) > 0).all()
            assert targets[0] >= 0 and targets[-1] < (lay.nnz if rank == 2
                                                      else N)
            assert ptr[0] == 0 and ptr[-1] == len(src) \
                and (numpy.diff(ptr) > 0).all()
            # every entry lands on the target of its (row, column) | dof,
            # ascending by facet position, then by ij, within a target
            for t, tg in enumerate(targets):
                row = int(numpy.searchsorted(rowptr, tg, side='right')) - 1
                keys = []
                for e in src[ptr[t]:ptr[t + 1]]:
                    ij, k = divmod(int(e), nf)
                    i, j = divmod(ij, nl) if rank == 2 else (ij, 0)
                    dofs = lay.cell_dofs[cells[k]]
                    if rank == 2:
                        assert (dofs[i], dofs[j]) == (row, cols[tg])
                    else:
                        assert dofs[i] == tg
                    keys.append((k, ij))
                assert keys == sorted(keys)
            if sel_args[1] == 'everywhere':
                full[rank] = set(targets)
                # all NL dofs of the owning cells take part
                want = set(lay.cell_dofs[cells].reshape(-1)) if rank == 1 \
                    else None
                assert want is None or want == full[rank]
            else:
                # a marker selection yields a subset of the full map
                assert 0 < len(targets) < len(full[rank])
                assert set(targets) <= full[rank]
    # a corner cell with two boundary edges feeds one nonzero from two facets
    counts = numpy.bincount(mesh.bfacet_cell, minlength=mesh.num_cells())
    corner = int(numpy.nonzero(counts == 2)[0][0])
    ks = numpy.nonzero(mesh.bfacet_cell == corner)[0]
    nf = len(mesh.bfacets)
    targets, ptr, src = ops.facet_map_host(mesh, lay, 2)
    where = numpy.empty(len(src), dtype=numpy.int64)
    where[src] = numpy.repeat(numpy.arange(len(targets)), numpy.diff(ptr))
    for ij in range(nl * nl):
        t0, t1 = (where[ij * nf + k] for k in ks)
        assert t0 == t1 and ptr[t0 + 1] - ptr[t0] >= 2
    targets, ptr, src = ops.facet_map_host(mesh, lay, 1)
    where = numpy.empty(len(src), dtype=numpy.int64)
    where[src] = numpy.repeat(numpy.arange(len(targets)), numpy.diff(ptr))
    for i in range(nl):
        assert where[i * nf + ks[0]] == where[i * nf + ks[1]]


def test_reference_evaluator_closed_forms():
    mesh = fem.UnitSquareMesh(3, 2)
    m, dsm = _marked(mesh)
    X = SpatialCoordinate(mesh)
    n = FacetNormal(mesh)
    for degree in (1, 2):
        V = fem.FunctionSpace(mesh, 'CG', degree)
        u, v = TrialFunction(V), TestFunction(V)
        # the basis sums to one: sum_i int v_i ds = the perimeter | the side
        assert abs(faref.vector(v * ds).sum() - 4.0) < 1e-14
        assert abs(faref.vector(v * dsm(2)).sum() - 1.0) < 1e-14
        assert abs(faref.matrix(u * v * ds).sum() - 4.0) < 1e-14
        # int x y v ds summed over i: int x y ds = 1/2 + 1/2
        assert abs(faref.vector(X[0] * X[1] * v * ds).sum() - 1.0) < 1e-14
        # Green: sum_j int dot(grad phi_j, n) v ds = 0 (the gradient of 1),
        # and with w = x the flux through the boundary of grad x . n
        A = faref.matrix(dot(grad(u), n) * v * ds)
        assert numpy.abs(A.dot(numpy.ones(V.N))).max() < 1e-13
        x = V.layout.dof_coords[:, 0]
        # int n_x v ds, summed over i: int n_x ds = 0; weighted by x: 1
        assert abs(A.dot(x).sum()) < 1e-13
        assert abs(x.dot(A.dot(x)) - 1.0) < 1e-13
        # rows of dofs in no boundary cell are empty
        touched = faref.touched_dofs(V)
        B = faref.matrix(u * v * ds)
        assert (numpy.abs(B).sum(axis=1).A1[~touched] == 0.0).all()
        # the extended nodes evaluate on facets
        c = conditional(gt(X[0], 1.0 / 3.0), 2.0, 0.0) * CellDiameter(mesh)
        h = numpy.hypot(1.0 / 3.0, 0.5)
        # x > 1/3 on the right side (1) and on 2/3 of the top and the bottom
        # (the points lie inside the edges, and the edges end at x = 1/3)
        assert abs(faref.vector(c * v * ds).sum() - 2.0 * h * 7.0 / 3.0) \
            < 1e-13
