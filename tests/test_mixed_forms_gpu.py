# -*- coding: utf-8 -*-
'''
Forms of test and trial functions on a Taylor-Hood space on the GPU
(flow_amd/fem/mixed.py, flow_form_rect_matrix): bits of the corners against
the vector and scalar forms, the coupling blocks entry by entry against the
host evaluator of tests/mixed_form_reference.py and against the oracle's
Stokes matrix, MixedMatrix.apply, assemble_system, and MINRES solves.
'''
import ctypes

import numpy
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from flow_amd import fem, _hip
from flow_amd.fem import (
    TestFunction, TrialFunction, TestFunctions, TrialFunctions, assemble,
    assemble_system, solve, dx, Measure, MeshFunction, SpatialCoordinate,
    FacetNormal, dot, inner, grad, div, sym,
    )
from flow_amd.fem import ops, mixed, reference
from flow_amd.fem.bcs import collect
from oracle import fem_oracle as orc

import mixed_form_reference as mref

pytestmark = pytest.mark.gpu

# the bound of tests/test_vector_forms_gpu.py against its host evaluator: the
# same element arithmetic with fewer columns
TOL = 1e-12
# field parity (README): no solve may differ by more
PARITY = 1e-7


@pytest.fixture(autouse=True)
def _switches_on():
    with fem.mixed_arguments(True), fem.vector_arguments(True), \
            fem.facet_arguments(True), fem.cell_subdomains(True):
        yield


class _Side(fem.SubDomain):
    def __init__(self, test):
        fem.SubDomain.__init__(self)
        self.test = test

    def inside(self, x, on_boundary):
        return on_boundary & self.test(x)


class _Region(fem.SubDomain):
    def inside(self, x, on_boundary):
        return x[0] < 0.5


def _meshes():
    return [fem.UnitSquareMesh(12, 9), fem.karman_channel(60, 14, fitted=True)]


def _space(mesh, kv, kp):
    return fem.FunctionSpace(
        mesh, fem.VectorElement('Lagrange', 'triangle', kv)
        * fem.FiniteElement('Lagrange', 'triangle', kp))


PAIRS = [(2, 1), (1, 1)]


def _err(got, ref, what=''):
    got = got.toarray() if hasattr(got, 'toarray') else numpy.asarray(got)
    ref = ref.toarray() if hasattr(ref, 'toarray') else numpy.asarray(ref)
    e = numpy.abs(got - ref).max() / numpy.abs(ref).max()
    print('%-60s %.2e' % (what, e))
    return e


def _host(t):
    return t.cpu().numpy().copy()


def _stokes(WP, mu):
    (u, p) = TrialFunctions(WP)
    (v, q) = TestFunctions(WP)
    return mu * inner(grad(u), grad(v)) * dx - p * div(v) * dx \
        - q * div(u) * dx


def test_corners_bitwise_and_repeatable(hip):
    for mesh in _meshes():
        x = SpatialCoordinate(mesh)
        for kv, kp in PAIRS:
            WP = _space(mesh, kv, kp)
            W, P = WP.sub(0), WP.sub(1)
            (u, p), (v, q) = TrialFunctions(WP), TestFunctions(WP)
            c = 1.0 + x[0] * x[1]
            a = c * inner(grad(u), grad(v)) * dx + dot(u, v) * dx \
                - p * div(v) * dx - q * div(u) * dx - 0.1 * c * p * q * dx
            A = assemble(a)
            A2 = assemble(a)
            uw, vw = TrialFunction(W), TestFunction(W)
            Au = assemble(c * inner(grad(uw), grad(vw)) * dx
                          + dot(uw, vw) * dx)
            pw, qw = TrialFunction(P), TestFunction(P)
            Ap = assemble(-0.1 * c * pw * qw * dx)
            for k in range(4):
                assert numpy.array_equal(_host(A.uu.plane(k)),
                                         _host(Au.plane(k)))
            assert numpy.array_equal(_host(A.pp.plane(0)), _host(Ap.plane(0)))
            for (name, B), (_, B2) in zip(A.blocks(), A2.blocks()):
                assert numpy.array_equal(_host(B.vals), _host(B2.vals)), name
            L = inner(c * x, v) * dx + c * q * dx
            b, b2 = assemble(L), assemble(L)
            bu = assemble(inner(c * x, vw) * dx)
            bp = assemble(c * qw * dx)
            assert numpy.array_equal(
                b.get_local(),
                numpy.concatenate([bu.get_local(), bp.get_local()]))
            assert numpy.array_equal(b.get_local(), b2.get_local())


def test_rect_kernel_equals_square_kernel_bitwise(hip):
    '''flow_form_rect_matrix with equal degrees and the space's own maps
    gives the bits of flow_form_matrix.'''
    from flow_amd.fem import forms
    lib = _hip.lib()
    for mesh in _meshes():
        x = SpatialCoordinate(mesh)
        for k in (1, 2):
            V = fem.FunctionSpace(mesh, 'CG', k)
            lay = V.layout
            uw, vw = TrialFunction(V), TestFunction(V)
            form = (1.0 + x[0]) * inner(grad(uw), grad(vw)) * dx \
                + uw.dx(0) * vw * dx
            want = assemble(form)
            total = None
            for _, part in form.terms():
                _, table = part.argument_table()
                q, scheme = ops._part_rule(part, None)
                for prog in forms.argument_programs(table, 2, False):
                    fs, keep = ops._form_struct(prog, mesh, q, False, scheme)
                    out = ops.value_plane(lay)
                    n = lay.nloc ** 2 * mesh.num_cells()
                    ss = ctypes.byref(ops.space_struct(lay))
                    _hip.check(lib.flow_form_rect_matrix(
                        ctypes.byref(ops.mesh_struct(mesh)), ss, ss,
                        ctypes.byref(fs), _hip.f64(ops.scratch(mesh, n), n),
                        _hip.f64(out, lay.nnz),
                        _hip.i32(lay.dev('cptr'), lay.nnz + 1),
                        _hip.i32(lay.dev('csrc'), n), lay.nnz, _hip.stream()))
                    total = out if total is None else ops.axpby(
                        1.0, out, 1.0, total)
            assert numpy.array_equal(_host(total[:lay.nnz]),
                                     _host(want.plane(0)))


def _markers(mesh):
    facets = MeshFunction('size_t', mesh, 1)
    facets.set_all(0)
    _Side(lambda x: x[0] < 1e-12).mark(facets, 1)
    cellm = MeshFunction('size_t', mesh, 2)
    cellm.set_all(0)
    _Region().mark(cellm, 1)
    return facets, cellm


def test_coupling_blocks_against_host_evaluator(hip):
    for mesh in _meshes():
        x = SpatialCoordinate(mesh)
        n = FacetNormal(mesh)
        facets, cellm = _markers(mesh)
        dsm = Measure('ds', domain=mesh, subdomain_data=facets)
        dxm = Measure('dx', domain=mesh, subdomain_data=cellm)
        for kv, kp in PAIRS:
            WP = _space(mesh, kv, kp)
            (u, p), (v, q) = TrialFunctions(WP), TestFunctions(WP)
            c = 1.0 + x[0] * x[1]
            cases = {
                '-q div u': -q * div(u) * dx,
                '-p div v': -p * div(v) * dx,
                'c(x) p v0': c * p * v[0] * dx,
                'grad p . v': dot(grad(p), v) * dx,
                'p v.n ds(1)': p * dot(v, n) * dsm(1),
                'alpha u.v + c q u1 dx(1)':
                    3.0 * dot(u, v) * dxm(1) + c * q * u[1] * dxm(1),
                'Stokes': _stokes(WP, fem.Constant(0.7)),
                }
            for name, form in cases.items():
                tag = '%d cells P%d/P%d %s' % (mesh.num_cells(), kv, kp, name)
                got = assemble(form).to_scipy()
                assert _err(got, mref.matrix(form), tag) < TOL


def test_stokes_matrix_against_oracle_and_transpose(hip):
    for mesh in _meshes():
        WP = _space(mesh, 2, 1)
        W, P = WP.sub(0), WP.sub(1)
        mu = 0.7
        A = assemble(_stokes(WP, fem.Constant(mu)))
        Wo = orc.Space(mesh.points, mesh.cell_vertices, W.layout.cell_dofs, 2,
                       W.N)
        Po = orc.Space(mesh.points, mesh.cell_vertices, P.layout.cell_dofs, 1,
                       P.N)
        # (the matrix of oracle.fem_oracle.stokes_solve, which does not
        # expose it: its K, B via _coo, and bmat)
        pts, w = orc.duffy_rule(4)
        _, gref = orc.basis(2, pts)
        gphi = Wo.phys_grad(gref)
        psi, _ = orc.basis(1, pts)
        wd = w[None, :] * numpy.abs(Wo.detJ)[:, None]
        Be = -numpy.einsum('cq,qi,cqja->ciaj', wd, psi, gphi)
        B = orc._coo(Po, Wo, Be[:, None, :, :, :], 1, 2)
        K = orc.stiffness_matrix(Wo)
        Aref = sp.bmat([[sp.block_diag([mu * K, mu * K]), B.T], [B, None]],
                       format='csr')
        assert _err(A.to_scipy(), Aref,
                    '%d cells Stokes vs oracle' % mesh.num_cells()) < TOL
        # pu[s] against the transpose of up[s]: the same cells and products,
        # but the kernel multiplies (w c psi_j) dphi_i in one and (w c dphi_i)
        # psi_j in the other, so single products differ in the last bit and
        # the sums by a few of them: bounded relative to the block's largest
        # entry by 2 ulp
        for s in range(2):
            up = A.up[s].to_scipy().toarray()
            pu = A.pu[s].to_scipy().toarray()
            d = numpy.abs(pu - up.T).max() / numpy.abs(up).max()
            print('pu%d vs up%d^T: %.2e (exact: %s)'
                  % (s, s, d, numpy.array_equal(pu, up.T)))
            assert d <= 2 * 2.0 ** -52


def test_apply_against_scipy(hip):
    rng = numpy.random.RandomState(5)
    for mesh in _meshes():
        x = SpatialCoordinate(mesh)
        for kv, kp in PAIRS:
            WP = _space(mesh, kv, kp)
            (u, p), (v, q) = TrialFunctions(WP), TestFunctions(WP)
            a = _stokes(WP, fem.Constant(0.7)) + dot(u, v) * dx \
                - (1.0 + x[0]) * p * q * dx
            A = assemble(a)
            S = A.to_scipy()
            xs = rng.standard_normal(A.size) * 10.0 ** rng.uniform(
                -3, 3, A.size)
            w = fem.Function(WP)
            w.set_array(xs)
            got = (A * w).get_local()
            want = S @ xs
            scale = abs(S) @ numpy.abs(xs)
            # one fp64 CSR-stream product of a row of len entries errs by at
            # most (len + c) 2^-53 sum |v| |x| (tests/test_fp64_streams_gpu.py,
            # c = 2 for its tile sums); a row of the mixed matrix adds up to
            # three block products (uu: one kind-2 product over two planes)
            rowlen = numpy.diff(S.indptr)
            bound = 3 * (rowlen + 2) * 2.0 ** -53 * scale
            worst = (numpy.abs(got - want) / numpy.maximum(bound, 1e-300)).max()
            print('apply P%d/P%d, %d cells: worst error / bound %.3g'
                  % (kv, kp, mesh.num_cells(), worst))
            assert worst <= 1.0


def _conditions(WP, mesh):
    (x0, y0), (x1, y1) = mesh.points.min(axis=0), mesh.points.max(axis=0)
    left = _Side(lambda x: x[0] < x0 + 1e-12)
    walls = _Side(lambda x: (x[1] < y0 + 1e-12) | (x[1] > y1 - 1e-12))
    right = _Side(lambda x: x[0] > x1 - 1e-12)
    return [
        fem.DirichletBC(WP.sub(0), fem.Expression(
            ('x[1]*(1.0 - x[1])', '0.25*x[0]'), degree=2), left),
        fem.DirichletBC(WP.sub(0).sub(1), fem.Constant(0.5), walls),
        fem.DirichletBC(WP.sub(1), fem.Constant(2.0), right),
        ]


def _sparse_err(got, ref, what):
    e = abs(got - ref).max() / abs(ref).max()
    print('%-60s %.2e' % (what, e))
    return e


def test_assemble_system_against_oracle_elimination(hip):
    for mesh in _meshes():
        x = SpatialCoordinate(mesh)
        for kv, kp in PAIRS:
            WP = _space(mesh, kv, kp)
            (u, p), (v, q) = TrialFunctions(WP), TestFunctions(WP)
            a = _stokes(WP, fem.Constant(0.7))
            L = inner(x, v) * dx + x[0] * q * dx
            bcs = _conditions(WP, mesh)
            A0, b0 = assemble(a).to_scipy(), assemble(L).get_local()
            A, b = assemble_system(a, L, bcs)
            dofs, vals, umask, pmask = mixed.mixed_bcs(bcs, WP)
            assert umask.any() and pmask.any() and not umask.all()
            Aref, bref_ = orc.symmetric_bc(A0, b0, dofs, vals)
            S = A.to_scipy()
            tag = '%d cells P%d/P%d assemble_system ' % (mesh.num_cells(), kv,
                                                        kp)
            assert _sparse_err(S, Aref, tag + 'A') < TOL
            assert _err(b.get_local(), bref_, tag + 'b') < TOL
            # eliminated rows and columns: exactly zero, diagonal exactly 1
            # (explicit zeros are dropped: one stored entry each)
            rows, cols = S[dofs].tocoo(), S[:, dofs].tocoo()
            for M in (rows, cols):
                assert M.nnz == len(dofs)
                assert (M.data == 1.0).all()
            assert numpy.array_equal(rows.col, dofs[rows.row])
            assert numpy.array_equal(cols.row, dofs[cols.col])


def test_assemble_system_symmetric_bit_for_bit(hip):
    '''The eliminated matrix of the (symmetric) reference form is symmetric
    bit for bit.  The element kernels alone do not give that: entry (i, j) is
    (w c dpsi_j) dphi_i and entry (j, i) is (w c dphi_i) dpsi_j, products that
    differ in the last bit (measured on an MI355X before assemble_system took
    the symmetric part, max |A - A^T| / max |A| on UnitSquareMesh(12, 9):
    P2/P1 1.14e-16, P1/P1 4.76e-18).  assemble_system therefore returns (A +
    A^T) / 2 of a structurally symmetric form (mixed.symmetric_part), and
    assemble(a) itself stays symmetric to that rounding only.'''
    worst = 0.0
    for mesh in _meshes():
        for kv, kp in PAIRS:
            WP = _space(mesh, kv, kp)
            a = _stokes(WP, fem.Constant(0.7))
            A, _ = assemble_system(a, None, _conditions(WP, mesh))
            S = A.to_scipy()
            d = abs(S - S.T).max() / abs(S).max()
            S0 = assemble(a).to_scipy()
            print('%d cells P%d/P%d asymmetry: assemble %.2e, assemble_system '
                  '%.2e' % (mesh.num_cells(), kv, kp,
                            abs(S0 - S0.T).max() / abs(S0).max(), d))
            worst = max(worst, d)
    assert worst == 0.0


def test_refusals_that_need_a_function(hip):
    mesh = fem.UnitSquareMesh(3, 2)
    WP = _space(mesh, 2, 1)
    (u, p), (v, q) = TrialFunctions(WP), TestFunctions(WP)
    w = fem.Function(WP)
    wu, wp = w.split()
    assert w.sub(0).data.data_ptr() == wu.data.data_ptr() == w.data.data_ptr()
    assert wp.data.data_ptr() == w.data.data_ptr() + 8 * WP.sub(0).size()
    assert w.split(True)[0].data.data_ptr() != w.data.data_ptr()
    F = inner(grad(wu), grad(v)) * dx - wp * div(v) * dx - q * div(wu) * dx
    with pytest.raises(NotImplementedError,
                       match='derivative with respect to a Function of a '
                             'vector, component or mixed space'):
        fem.derivative(F, w)
    with pytest.raises(NotImplementedError,
                       match='solve\\(F == 0\\) on a mixed space'):
        solve(F == 0, w, [])
    # what a Function is does not change when the switch goes off again
    with fem.mixed_arguments(False):
        assert fem.split(w)[1].function_space().same_as(WP.sub(1))
        assert w.value_dim() == 3 and w.sub(1).data.numel() == WP.sub(1).N
        with pytest.raises(AssertionError):
            fem.Function(WP)
    # 'two_level' without a Dirichlet dof on a velocity component
    a = _stokes(WP, fem.Constant(1.0)) + dot(u, v) * dx
    L = inner(fem.Constant((1.0, 0.0)), v) * dx
    pin = fem.DirichletBC(WP.sub(1), fem.Constant(0.0), 'on_boundary')
    with pytest.raises(ValueError, match='Dirichlet condition on every '
                                         'velocity component'):
        solve(a == L, w, [pin],
              solver_parameters={'preconditioner': 'two_level'})
    info = solve(a == L, w, [pin])
    assert info.iterations <= 1000


def _poiseuille(n=(8, 6), mu=0.7):
    mesh = fem.UnitSquareMesh(*n)
    WP = _space(mesh, 2, 1)
    inflow = fem.Expression(('x[1]*(1.0 - x[1])', '0.0'), degree=2)
    bcs = [fem.DirichletBC(WP.sub(0), inflow,
                           _Side(lambda x: x[0] < 1e-12)),
           fem.DirichletBC(WP.sub(0), fem.Constant((0.0, 0.0)), _Side(
               lambda x: (x[1] < 1e-12) | (x[1] > 1.0 - 1e-12)))]
    return mesh, WP, bcs, mu


def _rel(got, want):
    return numpy.abs(got - want).max() / numpy.abs(want).max()


# Measured on an MI355X on the first run of these tests, max-norm difference
# relative to max|u| and max|p| after MINRES at relative 1e-12 on the
# preconditioned residual (UnitSquareMesh(8, 6), P2/P1):
#   Poiseuille, exact solution      jacobi    u 2.82e-12  p 7.15e-12  (200 its)
#                                   two_level u 3.89e-12  p 6.18e-12  (162 its)
#   f != 0, pinned p, vs oracle LU  jacobi    u 1.34e-12  p 6.51e-12  (193 its)
#                                   two_level u 1.80e-12  p 1.03e-11  (159 its)
#                          preconditioner_form u 1.06e-12  p 6.38e-12  (227 its)
#   variable viscosity vs spsolve   jacobi    u 3.29e-12  p 1.09e-11  (246 its)
# The bounds are 10x the largest measured figure -- the stopping test sees the
# preconditioned norm -- and far below the field-parity bound.  (Measured
# again once assemble_system returned the symmetric part: u <= 3.88e-12, p <=
# 1.01e-11, iteration counts within 4 of the above; the bounds stay.)
SOLVE_BOUND_U = min(PARITY, 10 * 3.89e-12)
SOLVE_BOUND_P = min(PARITY, 10 * 1.09e-11)


def test_poiseuille_exact(hip):
    mesh, WP, bcs, mu = _poiseuille()
    (u, p), (v, q) = TrialFunctions(WP), TestFunctions(WP)
    a = _stokes(WP, fem.Constant(mu))
    L = inner(fem.Constant((0.0, 0.0)), v) * dx
    W, P = WP.sub(0), WP.sub(1)
    xu, xp = W.layout.dof_coords, P.layout.dof_coords
    ue = numpy.concatenate([xu[:, 1] * (1 - xu[:, 1]), 0 * xu[:, 0]])
    pe = 2 * mu * (1 - xp[:, 0])
    for prm in ({}, {'preconditioner': 'two_level'}):
        w = fem.Function(WP)
        info = solve(a == L, w, bcs, solver_parameters=prm)
        uh, ph = w.split(True)
        eu, ep = _rel(uh.array(), ue), _rel(ph.array(), pe)
        print('Poiseuille %r: %r, u %.2e p %.2e' % (prm, info, eu, ep))
        assert info.iterations <= 1000
        assert eu < SOLVE_BOUND_U and ep < SOLVE_BOUND_P


def test_solves_against_sparse_lu(hip):
    mesh, WP, bcs, mu = _poiseuille()
    W, P = WP.sub(0), WP.sub(1)
    x = SpatialCoordinate(mesh)
    (u, p), (v, q) = TrialFunctions(WP), TestFunctions(WP)
    f = fem.Expression(('sin(3.0*x[1])', 'x[0]*x[1]'), degree=2)
    pin = fem.DirichletBC(WP.sub(1), fem.Constant(0.0), _Side(
        lambda x: x[0] > 1.0 - 1e-12))
    a = _stokes(WP, fem.Constant(mu))
    L = inner(f, v) * dx
    # (b) the oracle's Stokes solve (sparse LU)
    Wo = orc.Space(mesh.points, mesh.cell_vertices, W.layout.cell_dofs, 2, W.N)
    Po = orc.Space(mesh.points, mesh.cell_vertices, P.layout.cell_dofs, 1, P.N)
    X = fem.cell_lattice_points(mesh, 2)
    nc, nl = X.shape[:2]
    fv = f.eval(X.reshape(-1, 2).T)
    flat = (reference.lattice(2), numpy.ascontiguousarray(
        fv.reshape(2, nc, nl).transpose(1, 2, 0)))
    uo, po = orc.stokes_solve(Wo, Po, flat, mu, collect(bcs, W.size()),
                              collect([pin], P.N))
    prec = mu * inner(grad(u), grad(v)) * dx - p * q * dx
    for prm in ({}, {'preconditioner': 'two_level'},
                {'preconditioner_form': prec}):
        w = fem.Function(WP)
        info = solve(a == L, w, bcs + [pin], solver_parameters=prm)
        uh, ph = w.split(True)
        eu, ep = _rel(uh.array(), uo), _rel(ph.array(), po)
        print('Stokes vs oracle LU %s: %r, u %.2e p %.2e'
              % (sorted(prm), info, eu, ep))
        assert info.iterations <= 1000
        assert eu < SOLVE_BOUND_U and ep < SOLVE_BOUND_P
    # (d) variable viscosity, which stokes.py cannot do
    nu = 1.0 + x[0]
    a = 2.0 * nu * inner(sym(grad(u)), sym(grad(v))) * dx - p * div(v) * dx \
        - q * div(u) * dx
    A, b = assemble_system(a, L, bcs + [pin])
    xs = spla.spsolve(A.to_scipy().tocsc(), b.get_local())
    w = fem.Function(WP)
    info = solve(a == L, w, bcs + [pin])
    n2 = W.size()
    eu, ep = _rel(w.array()[:n2], xs[:n2]), _rel(w.array()[n2:], xs[n2:])
    print('variable viscosity vs spsolve: %r, u %.2e p %.2e' % (info, eu, ep))
    assert eu < SOLVE_BOUND_U and ep < SOLVE_BOUND_P
    # a non-symmetric form assembles but is not solved
    a = _stokes(WP, fem.Constant(mu)) + 2.0 * q * div(u) * dx
    A, b = assemble_system(a, L, bcs + [pin])
    assert A.to_scipy().shape == (WP.size(), WP.size())
    with pytest.raises(NotImplementedError, match='non-symmetric'):
        solve(a == L, fem.Function(WP), bcs + [pin])
