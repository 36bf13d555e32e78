# -*- coding: utf-8 -*-
'''
Cell subdomains, dx(k), on the HIP path (flow_form_cells_functional / _values /
_matrix / _vector, the cell contribution map; ops.assemble / assemble_system /
solve, Newton, vector spaces, cell_indicator, Eigenmodes): against the numpy
reference of tests/cell_subdomain_reference.py, bit identities with plain dx,
exact zeros off the selected cells, partitions, and solves.  Meshes and
selections are those of tests/test_cell_subdomains_host.py: the unit square
(216 cells, fewer lanes than one block) and the fitted Karman channel (a
hole, graded cells, several blocks); a disc whose circle cuts cells, the first
kBlock + 1 cells, one cell, all cells, nobody.

Bounds.  Against the host reference: 1e-12 of the largest entry, the bound of
tests/test_bilinear_forms_gpu.py for the same comparison over whole dx.
Partition: 1e-13 relative (three sums in another order).  Linear solves
against sparse LU and Newton against the host Newton: 1e-7 relative l2, the
bounds of tests/test_bilinear_forms_gpu.py and tests/newton_reference.py.
Eigenvalues: the Krylov-Weinstein radius of tests/test_eigen_gpu.py.  The
central difference of the block-Newton Jacobian: 100 eps max|F| / h, the bound
of tests/test_vector_newton_host.py (see test_block_newton_forchheimer).
'''
import numpy
import pytest

from flow_amd import device, fem
from flow_amd.fem import (
    TestFunction, TrialFunction, assemble, dx, Measure, MeshFunction,
    SpatialCoordinate, conditional, gt, sin, sqrt, dot, inner, grad, sym, tr,
    Identity, derivative,
    )
from flow_amd.fem import ops

import cell_subdomain_reference as csref
import eigen_reference as eref
import newton_reference as nref
import vector_newton_reference as vnref
from test_cell_subdomains_host import cases, NOTHING

pytestmark = pytest.mark.gpu

EPS = numpy.finfo(float).eps


@pytest.fixture(autouse=True)
def _cell_subdomains_on():
    '''Cell subdomains are off by default: on for these tests only.'''
    with fem.cell_subdomains(True):
        yield


@pytest.fixture(scope='module')
def CASES():
    with fem.cell_subdomains(True):
        return cases()


def _spaces(mesh):
    return [fem.FunctionSpace(mesh, 'CG', k) for k in (1, 2)]


def _field(V, f):
    u = fem.Function(V)
    xy = V.layout.dof_coords
    u.set_array(f(xy[:, 0], xy[:, 1]))
    return u


def _err(got, ref, what=''):
    '''max entrywise error relative to max|entry| (printed: the measured
    figure is part of the record).'''
    got = got.toarray() if hasattr(got, 'toarray') else numpy.asarray(got)
    ref = ref.toarray() if hasattr(ref, 'toarray') else numpy.asarray(ref)
    e = numpy.abs(got - ref).max() / numpy.abs(ref).max()
    print('%-56s %.2e' % (what, e))
    return e


def _vals(A):
    return A.plane(0).cpu().numpy().copy()


def _coefficient(mesh):
    '''A variable coefficient with a P2 Function, a conditional, an
    Expression and SpatialCoordinate (NF > 0, the extended interpreter).'''
    X = SpatialCoordinate(mesh)
    P2 = fem.FunctionSpace(mesh, 'CG', 2)
    th = _field(P2, lambda x, y: 0.5 + numpy.sin(3 * x) * y)
    ex = fem.Expression('exp(0.3*x[0]) + x[1]*x[1]', degree=2)
    return conditional(gt(th, 0.5), th * th, 1.0 + X[0] * X[0]) + ex, th


def _forms(mesh, V, d):
    '''{rank: [(name, form)]} over the measure d.'''
    u, v = TrialFunction(V), TestFunction(V)
    c, th = _coefficient(mesh)
    kappa = fem.Constant(2.5)
    w = _field(V, lambda x, y: numpy.cos(2 * x) + x * y)
    return {
        0: [('stiffness energy', kappa * inner(grad(w), grad(w)) * d),
            ('mass', w * w * d),
            ('variable', c * (w * w + th.dx(0)**2) * d)],
        1: [('stiffness action', kappa * inner(grad(w), grad(v)) * d),
            ('mass', w * v * d),
            ('variable', (c * v + th * v.dx(1)) * d)],
        2: [('stiffness', kappa * inner(grad(u), grad(v)) * d),
            ('mass', u * v * d),
            ('variable', (c * inner(grad(u), grad(v)) + th.dx(1) * u * v
                          + sin(SpatialCoordinate(mesh)[1]) * u * v.dx(0)) * d)],
        }


def _assembled(form):
    if form.rank == 0:
        return numpy.array([assemble(form)])
    if form.rank == 1:
        return assemble(form).get_local()
    return _vals(assemble(form))


def test_against_host_reference(hip, CASES):
    for tag, mesh, sels in CASES:
        for V in _spaces(mesh):
            for name, m, k in sels[:3]:
                d = Measure('dx', domain=mesh, subdomain_data=m)(k)
                for rank, items in sorted(_forms(mesh, V, d).items()):
                    for fname, form in items:
                        what = '%s P%d %s rank %d %s' % (tag, V.degree, name,
                                                         rank, fname)
                        if rank == 0:
                            # (the integrands of rank 0 are positive: the
                            # value is its own scale)
                            e = _err([assemble(form)],
                                     [csref.functional(form)], what)
                        elif rank == 1:
                            e = _err(assemble(form).get_local(),
                                     csref.vector(form), what)
                        else:
                            e = _err(assemble(form).to_scipy(),
                                     csref.matrix(form), what)
                        assert e < 1e-12


def test_bits(hip, CASES):
    for tag, mesh, sels in CASES:
        name, every, k = sels[3]
        assert name == 'all'
        dall = Measure('dx', domain=mesh, subdomain_data=every)(k)
        dsome = Measure('dx', domain=mesh, subdomain_data=sels[0][1])(1)
        for V in _spaces(mesh):
            whole, listed, some = (_forms(mesh, V, d)
                                   for d in (dx(mesh), dall, dsome))
            for rank in (0, 1, 2):
                for (fname, f0), (_, f1), (_, f2) in zip(
                        whole[rank], listed[rank], some[rank]):
                    # every cell marked: the bits of plain dx
                    a, b = _assembled(f0), _assembled(f1)
                    assert numpy.array_equal(a, b), (tag, V.degree, rank, fname)
                    assert numpy.abs(a).max() > 0.0
                    # two calls: the same bits
                    s = _assembled(f2)
                    assert numpy.array_equal(s, _assembled(f2))
    # re-marking and marking back: the bits return
    tag, mesh, sels = CASES[0]
    m = MeshFunction('size_t', mesh, 2, 0)
    m.set_where(numpy.arange(mesh.num_cells()) % 3 == 0, 1)
    d = Measure('dx', domain=mesh, subdomain_data=m)(1)
    V = fem.FunctionSpace(mesh, 'CG', 2)
    forms_ = [f for items in _forms(mesh, V, d).values() for _, f in items[2:]]
    before = [_assembled(f) for f in forms_]
    m[1] = 1
    m[0] = 0
    changed = [_assembled(f) for f in forms_]
    assert all(not numpy.array_equal(a, b) for a, b in zip(before, changed))
    for f, got in zip(forms_, changed):
        if f.rank == 1:
            assert _err(got, csref.vector(f), 're-marked rank 1') < 1e-12
    m[1] = 0
    m[0] = 1
    after = [_assembled(f) for f in forms_]
    assert all(numpy.array_equal(a, b) for a, b in zip(before, after))


def test_exact_zeros(hip, CASES):
    for tag, mesh, sels in CASES:
        for V in _spaces(mesh):
            u, v = TrialFunction(V), TestFunction(V)
            for name, m, k in sels[:3]:
                d = Measure('dx', domain=mesh, subdomain_data=m)(k)
                keep = numpy.asarray(m.array()) == k
                on = csref.touched(V, keep, 1)
                on2 = csref.touched(V, keep, 2)
                # (on the square the first kBlock + 1 cells are all cells)
                assert on.any() and on2.any()
                assert keep.all() or not (on.all() or on2.all())
                b = assemble(v * d).get_local()
                assert (b[~on] == 0.0).all() and (b[on] != 0.0).any()
                A = _vals(assemble((u * v + inner(grad(u), grad(v))) * d))
                assert A.shape == (V.layout.nnz,)
                assert (A[~on2] == 0.0).all() and (A[on2] != 0.0).any()
            m = sels[0][1]
            d = Measure('dx', domain=mesh, subdomain_data=m)(NOTHING)
            assert assemble(1.0 * d) == 0.0
            b = assemble(v * d).get_local()
            assert b.shape == (V.N,) and (b == 0.0).all()
            A = assemble(u * v * d)
            assert (_vals(A) == 0.0).all()


def test_partition(hip, CASES):
    for tag, mesh, sels in CASES:
        nc = mesh.num_cells()
        m = MeshFunction('size_t', mesh, 2, 0)
        m.set_where(numpy.arange(nc) % 3 == 1, 1)
        m.set_where(numpy.arange(nc) % 7 == 2, 2)
        assert set(numpy.unique(m.array())) == {0, 1, 2}
        dxm = Measure('dx', domain=mesh, subdomain_data=m)
        for V in _spaces(mesh):
            for rank in (0, 1, 2):
                fname, whole = _forms(mesh, V, dx(mesh))[rank][2]
                parts = [_assembled(_forms(mesh, V, dxm(k))[rank][2][1])
                         for k in (0, 1, 2)]
                total = parts[0] + parts[1] + parts[2]
                ref = _assembled(whole)
                e = _err(total, ref, '%s P%d rank %d partition'
                         % (tag, V.degree, rank))
                assert e < 1e-13


class _Right(fem.SubDomain):
    def inside(self, x, on_boundary):
        return x[0] >= 0.5 - 1e-12


def _halves(mesh):
    m = MeshFunction('size_t', mesh, 2, 0)
    _Right().mark(m, 1)
    mid = mesh.points[mesh.cell_vertices].mean(axis=1)
    # the interface is a mesh line: the halves split the cells exactly
    assert numpy.array_equal(m.array() == 1, mid[:, 0] > 0.5)
    return m


def test_two_materials(hip):
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla
    mesh = fem.UnitSquareMesh(12, 9)
    dxm = Measure('dx', domain=mesh, subdomain_data=_halves(mesh))
    for V in _spaces(mesh):
        u, v = TrialFunction(V), TestFunction(V)
        k0, k1 = fem.Constant(1.0), fem.Constant(10.0)
        a = k0 * inner(grad(u), grad(v)) * dxm(0) \
            + k1 * inner(grad(u), grad(v)) * dxm(1)
        L = fem.Constant(1.0) * v * dx
        bcs = [fem.DirichletBC(V, 0.0, 'on_boundary')]
        uh = fem.Function(V)
        info = fem.solve(a == L, uh, bcs)
        assert info.method == 'cg'
        dofs, g = fem.bcs.collect(bcs, V.N)
        keep = numpy.ones(V.N)
        keep[dofs] = 0.0
        K = sp.diags(keep)
        Aref = K.dot(csref.matrix(a)).dot(K) + sp.diags(1.0 - keep)
        bref_ = keep * csref.vector(L)
        A, b = fem.assemble_system(a, L, bcs)
        assert _err(A.to_scipy(), Aref, 'P%d system A' % V.degree) < 1e-12
        assert _err(b.get_local(), bref_, 'P%d system b' % V.degree) < 1e-12
        ref = spla.splu(Aref.tocsc()).solve(bref_)
        e = numpy.linalg.norm(uh.array() - ref) / numpy.linalg.norm(ref)
        print('two materials P%d: %r, rel l2 vs splu %.2e'
              % (V.degree, info, e))
        assert e < 1e-7


def _quasilinear(V, m):
    '''kappa(u) = 1 + u^2 in dx(1) only, linear elsewhere.'''
    dxm = Measure('dx', domain=V.mesh(), subdomain_data=m)
    u = _field(V, lambda x, y: 0.3 * numpy.sin(3.0 * x) * numpy.cos(2.0 * y))
    v = TestFunction(V)
    F = (1 + u**2) * inner(grad(u), grad(v)) * dxm(1) \
        + inner(grad(u), grad(v)) * dxm(0) - fem.Constant(8.0) * v * dx
    bcs = [fem.DirichletBC(V, 0.0, 'on_boundary')]
    return u, F, bcs


def test_newton(hip, monkeypatch):
    mesh = fem.UnitSquareMesh(12, 9)
    m = _halves(mesh)
    # newton_reference.host_newton with the masked reference matrices
    monkeypatch.setattr(nref, 'bref', csref)
    for V in _spaces(mesh):
        u, F, bcs = _quasilinear(V, m)
        J = derivative(F, u)
        asm = ops.NewtonAssembler(J, F, V)
        assert asm.route == 'by_parts' and not asm.fused
        assert [j.kind for j in asm.jobs] == [
            'cells_matrix', 'cells_matrix', 'cells_vector', 'cells_vector',
            'vector']
        A, b = asm.assemble()
        assert _err(A.to_scipy(), csref.matrix(J), 'P%d J' % V.degree) < 1e-12
        assert _err(b.cpu().numpy(), csref.vector(F), 'P%d F' % V.degree) \
            < 1e-12
        assert numpy.array_equal(_vals(A), _vals(assemble(J)))
        assert numpy.array_equal(b.cpu().numpy(), assemble(F).get_local())
        info = fem.solve(F == 0, u, bcs, J=J)
        assert info.converged and info.route == 'by_parts' and not info.fused
        ur, Fr, bcr = _quasilinear(V, m)
        res, its = nref.host_newton(Fr, ur, bcr, derivative(Fr, ur))
        print('P%d residuals, device: %s' % (V.degree, info.residuals))
        print('P%d residuals, host:   %s' % (V.degree, res))
        assert info.iterations == its
        e = numpy.linalg.norm(u.array() - ur.array()) \
            / numpy.linalg.norm(ur.array())
        print('quasilinear in dx(1) P%d: %r; rel l2 vs host Newton %.2e'
              % (V.degree, info, e))
        assert e < 1e-7
        assert numpy.abs(u.array()).max() > 0.05


def test_vector_space(hip):
    mesh = fem.UnitSquareMesh(12, 9)
    m = _halves(mesh)
    dxm = Measure('dx', domain=mesh, subdomain_data=m)
    with fem.vector_arguments(True):
        for degree in (1, 2):
            W = fem.VectorFunctionSpace(mesh, 'CG', degree)
            u, v = TrialFunction(W), TestFunction(W)

            def sigma(w, mu, lam):
                return 2.0 * mu * sym(grad(w)) + lam * tr(sym(grad(w))) \
                    * Identity(2)

            a = inner(sigma(u, fem.Constant(1.3), fem.Constant(0.7)),
                      sym(grad(v))) * dxm(0) \
                + inner(sigma(u, fem.Constant(4.0), fem.Constant(2.5)),
                        sym(grad(v))) * dxm(1)
            f = fem.Expression(('sin(x[0])*x[1]', '1.0 + x[0]'), degree=3)
            L = dot(f, v) * dxm(1) - dot(f, v) * dxm(0)
            A = assemble(a)
            assert A.kind == 2
            ref = csref.matrix(a)
            S = A.to_scipy()
            tag = 'elasticity P%d ' % degree
            assert _err(S, ref, tag + 'two Lame pairs') < 1e-12
            # the four planes, one by one
            N = W.N
            for p in range(4):
                r, s = divmod(p, 2)
                blk = ref[r * N:(r + 1) * N, s * N:(s + 1) * N]
                got = S[r * N:(r + 1) * N, s * N:(s + 1) * N]
                assert _err(got, blk, tag + 'plane %d' % p) < 1e-12
            assert _err(assemble(L).get_local(), csref.vector(L),
                        tag + 'load') < 1e-12
            assert numpy.array_equal(A.vals.cpu().numpy(),
                                     assemble(a).vals.cpu().numpy())
            # block Newton with a dx(k) Forchheimer term: the held assembler
            # against the host reference and against assemble()
            with fem.vector_derivatives(True):
                U = fem.Function(W)
                xy = W.layout.dof_coords
                U.set_array(numpy.concatenate(
                    [1.5 + 0.5 * numpy.sin(3.0 * xy[:, 0]),
                     0.5 - xy[:, 0] * xy[:, 1]]))
                s = sqrt(dot(U, U) + 1e-8)
                F = (0.1 * inner(grad(U), grad(v)) + 2.0 * dot(U, v)) * dx \
                    + 1.5 * s * dot(U, v) * dxm(1) - dot(f, v) * dx
                J = derivative(F, U)
                asm = ops.NewtonAssembler(J, F, W)
                assert asm.route == 'by_parts' and not asm.fused
                assert 'cells_matrix' in [j.kind for j in asm.jobs]
                for call in range(2):
                    A, b = asm.assemble()
                    assert numpy.array_equal(A.vals.cpu().numpy(),
                                             assemble(J).vals.cpu().numpy())
                    assert numpy.array_equal(b.cpu().numpy(),
                                             assemble(F).get_local())
                assert _err(A.to_scipy(), csref.matrix(J), tag + 'J') < 1e-12
                assert _err(b.cpu().numpy(), csref.vector(F), tag + 'F') \
                    < 1e-12


def _brinkman_forchheimer(W, m):
    """Brinkman flow with a Forchheimer drag beta |u| u in dx(1) only (a porous
    insert), |u| = sqrt(dot(u, u) + 1e-8) as tests/vector_newton_reference.py
    writes it; the state has |u| >= 0.5."""
    mesh = W.mesh()
    dxm = Measure('dx', domain=mesh, subdomain_data=m)
    u = vnref.state(W)
    v = TestFunction(W)
    mu, alpha, beta = fem.Constant(0.1), fem.Constant(2.0), fem.Constant(1.5)
    f = fem.Expression(vnref.SOURCE, degree=2)
    s = sqrt(dot(u, u) + 1e-8)
    F = (mu * inner(grad(u), grad(v)) + alpha * dot(u, v) - dot(f, v)) * dx \
        + beta * s * dot(u, v) * dxm(1)
    bcs = [fem.DirichletBC(W.sub(0), fem.Constant(1.0), 'on_boundary')]
    return u, F, bcs


def test_block_newton_forchheimer(hip, monkeypatch):
    """J d of derivative(F, u), assembled on the device, against the central
    difference (F(u + h d) - F(u - h d)) / 2h of the host reference's
    residual, h = 1e-3, with the bound of tests/test_vector_newton_host.py:
    100 eps max|F| / h (the rounding of the two residuals over h).

    That file's form is quadratic, so its quotient has no truncation error;
    the drag g(u) = |u| u is not.  The quotient's truncation is h^2 / 6
    D^3 F(u)[d, d, d]: entry i is at most h^2 / 6 beta max|D^3 g| |d|^3 int
    |phi_i|, with |D^3 g| <= 3 / |u| <= 6 on the state (|u| >= 0.5).  The
    direction is therefore taken SMALL, d uniform in [-delta, delta] with delta
    = 1e-2 (|d| <= 1.42 delta per point): the truncation is then at most
    1.7e-7 * 1.5 * 6 * 2.9e-6 int |phi_i| = 4.4e-12 int |phi_i|, against a bound
    of 2.2e-11 max|F| with max|F| of the order (alpha |u| + beta |u|^2) int
    phi_i ~ 4 int phi_i -- a factor 20 below it --, while J d itself is of
    the order delta (alpha + 2 beta |u|) int phi_i = 5e-2 int phi_i: the
    check resolves J d to a relative 2e-9, and a Jacobian without the dx(1)
    term would miss by 1e-2 int phi_i.  The same quotient of the DEVICE's
    residuals is held to the same bound.  The measured errors are printed.

    Then solve(F == 0) -- block Newton steps by parts -- against the host
    Newton with the masked reference matrices at 1e-7 relative l2, the bound
    of tests/test_vector_newton_gpu.py."""
    h, delta = 1.0e-3, 1.0e-2
    mesh = fem.UnitSquareMesh(12, 9)
    m = _halves(mesh)
    # vector_newton_reference.host_newton with the masked reference
    monkeypatch.setattr(vnref, 'vref', csref)
    with fem.vector_arguments(True), fem.vector_derivatives(True):
        for degree in (1, 2):
            W = fem.VectorFunctionSpace(mesh, 'CG', degree)
            u, F, bcs = _brinkman_forchheimer(W, m)
            J = derivative(F, u)
            assert [p.subdomain_id for _, p in J.terms()] == ['everywhere', 1]
            d = numpy.random.RandomState(3).uniform(-delta, delta, W.size())
            Jd = assemble(J).to_scipy().dot(d)
            u0 = u.array().copy()
            fd_host = vnref.central_difference(F, u, d, h)
            u.set_array(u0 + h * d)
            fp = assemble(F).get_local()
            u.set_array(u0 - h * d)
            fm = assemble(F).get_local()
            u.set_array(u0)
            fd_dev = (fp - fm) / (2.0 * h)
            bound = 100.0 * EPS * numpy.abs(csref.vector(F)).max() / h
            for name, fd in (('host', fd_host), ('device', fd_dev)):
                e = numpy.abs(Jd - fd).max()
                print('P%d |J d - central difference (%s F)| = %.2e, bound '
                      '%.2e, max|J d| %.2e' % (degree, name, e, bound,
                                               numpy.abs(Jd).max()))
                assert e < bound
            # the drag's part of J d is far above the bound: the check sees it
            drag = csref.matrix(J.terms()[1][1]).dot(d)
            assert numpy.abs(drag).max() > 1e3 * bound
            info = fem.solve(F == 0, u, bcs)
            assert info.converged and info.route == 'by_parts'
            assert not info.fused and info.iterations >= 1
            ur, Fr, bcr = _brinkman_forchheimer(W, m)
            res, its = vnref.host_newton(Fr, ur, bcr)
            e = numpy.linalg.norm(u.array() - ur.array()) \
                / numpy.linalg.norm(ur.array())
            print('Forchheimer in dx(1) P%d: %r (host: %d iterations); rel '
                  'l2 %.2e' % (degree, info, its, e))
            assert info.iterations == its
            assert e < 1e-7


def test_cell_indicator(hip, CASES):
    for tag, mesh, sels in CASES:
        V = fem.FunctionSpace(mesh, 'CG', 2)
        for name, m, k in sels:
            d = Measure('dx', domain=mesh, subdomain_data=m)(k)
            fname, form = _forms(mesh, V, d)[0][2]
            got = device.to_host(fem.cell_indicator(form)).numpy()
            ref = csref.cell_values(form)
            keep = numpy.asarray(m.array()) == k
            assert (got[~keep] == 0.0).all()
            if keep.any():
                assert _err(got, ref, '%s %s indicator' % (tag, name)) < 1e-12
                assert (got[keep] != 0.0).any()
            # a signed sum with a whole-mesh part
            both = form - _forms(mesh, V, dx(mesh))[0][1][1]
            got = device.to_host(fem.cell_indicator(both)).numpy()
            ref = csref.cell_values(both.terms()[0][1]) \
                - csref.cell_values(both.terms()[1][1])
            assert _err(got, ref, '%s %s indicator of a sum' % (tag, name)) \
                < 1e-12


def test_eigenmodes(hip):
    k = 3
    mesh = fem.UnitSquareMesh(12, 9)
    dxm = Measure('dx', domain=mesh, subdomain_data=_halves(mesh))
    for V in _spaces(mesh):
        u, v = TrialFunction(V), TestFunction(V)
        a = inner(grad(u), grad(v)) * dxm(0) \
            + 10 * inner(grad(u), grad(v)) * dxm(1)
        bcs = [fem.DirichletBC(V, 0.0, 'on_boundary')]
        r = fem.Eigenmodes(a, None, bcs).solve(k, rtol=1e-9, maxit=400)
        assert r.converged.all()
        A, M = csref.matrix(a), csref.matrix(u * v * dx)
        isbc = numpy.zeros(V.N, dtype=bool)
        isbc[fem.bcs.collect(bcs, V.N)[0]] = True
        want, _ = eref.smallest(A, M, isbc, k + 2)
        lmin = eref.mass_lambda_min(M, isbc)
        X = numpy.stack([device.to_host(x.data).numpy() for x in r.modes],
                        axis=1)
        assert (X[isbc, :] == 0.0).all()
        f = (~isbc).astype(float)[:, None]
        MX = f * M.dot(X)
        R = f * A.dot(X) - MX * r.values[None, :]
        rn = numpy.sqrt((R * R).sum(axis=0))
        xm = numpy.sqrt((X * MX).sum(axis=0))
        radius = rn / (numpy.sqrt(lmin) * xm) + 1e3 * EPS * abs(want[k - 1])
        print('P%d values %s\nreference %s\nradius %s'
              % (V.degree, r.values, want[:k], radius))
        assert eref.match_once(r.values, want, radius) == list(range(k))
        assert (numpy.abs(r.values - want[:k]) <= radius).all()
