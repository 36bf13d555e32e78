# -*- coding: utf-8 -*-
'''
Test and trial functions under ds on the HIP path (flow_form_facet_matrix,
flow_form_facet_vector, the facet contribution map; ops.assemble /
assemble_system / solve, Newton, Eigenmodes): against the numpy evaluator of
tests/facet_argument_reference.py, identities that tie the new kernels to the
facet functionals, exact zeros off the selected facets' cells, bit
reproducibility, and solves.  Meshes stay small: the unit square (42 boundary
facets, fewer lanes than one block at P1, corner cells with two boundary
edges) and the fitted Karman channel (a hole, more lanes than one block).

Bounds.  Against the host evaluator: 1e-12 of the largest entry, the bound of
tests/test_bilinear_forms_gpu.py for the same comparison over dx.  Linear
solves against sparse LU and Newton against the host Newton: 1e-7 relative
l2, the bounds of that file and of tests/test_nonlinear_forms_gpu.py.  The
central difference of the radiation residual: see test_newton_radiation.
Eigenvalues: the Krylov-Weinstein radius of tests/test_eigen_gpu.py.
'''
import numpy
import pytest

from flow_amd import device, fem, karman
from flow_amd.fem import (
    TestFunction, TrialFunction, assemble, dx, ds, Measure, MeshFunction,
    FacetNormal, SpatialCoordinate, CellDiameter, conditional, gt, sin, dot,
    inner, grad, lhs, rhs, derivative, as_vector,
    )

import bilinear_reference as bref
import eigen_reference as eref
import facet_argument_reference as faref

pytestmark = pytest.mark.gpu

EPS = numpy.finfo(float).eps
CYLINDER, WALL, NOTHING = 5, 3, 99


@pytest.fixture(autouse=True)
def _facet_arguments_on():
    '''Arguments under ds are off by default: on for these tests only.'''
    with fem.facet_arguments(True):
        yield


class _Side(fem.SubDomain):
    def __init__(self, test):
        fem.SubDomain.__init__(self)
        self.test = test

    def inside(self, x, on_boundary):
        return on_boundary & self.test(x)


def _square_markers(mesh):
    '''1 left, 2 right, 3 top; the bottom stays 0.'''
    m = MeshFunction('size_t', mesh, 1, 0)
    _Side(lambda x: x[0] < 1e-12).mark(m, 1)
    _Side(lambda x: x[0] > 1.0 - 1e-12).mark(m, 2)
    _Side(lambda x: x[1] > 1.0 - 1e-12).mark(m, 3)
    return m


def _cases():
    '''[(tag, mesh, markers, ids)]: ids = (a curved or short selection, one
    wall, nothing).'''
    sq = fem.UnitSquareMesh(12, 9)
    ch = fem.karman_channel(60, 14, fitted=True)
    m = MeshFunction('size_t', ch, 1, 0)
    karman.LowerBoundary().mark(m, WALL)
    karman.ObstacleBoundary().mark(m, CYLINDER)
    return [('square', sq, _square_markers(sq), (2, 3, NOTHING)),
            ('channel', ch, m, (CYLINDER, WALL, NOTHING))]


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
    print('%-52s %.2e' % (what, e))
    return e


def _vals(A):
    return A.plane(0).cpu().numpy()


def _forms(mesh, V, dsm, k):
    '''[(name, form)]: the forms of the comparison with the host evaluator.'''
    u, v = TrialFunction(V), TestFunction(V)
    n = FacetNormal(mesh)
    X = SpatialCoordinate(mesh)
    P2 = fem.FunctionSpace(mesh, 'CG', 2)
    th = _field(P2, lambda x, y: 0.5 + numpy.sin(3 * x) * y)
    ex = fem.Expression('exp(x[0]) + x[1]*x[1]', degree=2)
    g, h, uinf = fem.Constant(1.7), fem.Constant(3.0), fem.Constant(0.5)
    gamma = fem.Constant(10.0)
    robin = h * (u - uinf) * v * ds(mesh)
    nitsche = -dot(grad(u), n) * v * ds(mesh) - u * dot(grad(v), n) * ds(mesh) \
        + gamma / CellDiameter(mesh) * u * v * ds(mesh)
    c = conditional(gt(th, 0.5), th * th, 1.0 + X[0] * X[0]) + ex
    return [('u v ds', u * v * ds(mesh)),
            ('g v ds(k)', g * v * dsm(k)),
            ('Robin lhs', lhs(robin)), ('Robin rhs', rhs(robin)),
            ('Nitsche', nitsche),
            ('variable matrix', (c * u * v + th.dx(1) * dot(grad(u), n) * v
                                 + sin(X[1]) * u * v.dx(0)) * dsm(k)),
            ('variable vector', (c * v + ex * dot(grad(v), n) * th) * dsm(k))]


def test_against_host_reference(hip):
    for tag, mesh, m, ids in _cases():
        dsm = Measure('ds', domain=mesh, subdomain_data=m)
        for V in _spaces(mesh):
            for name, form in _forms(mesh, V, dsm, ids[0]):
                what = '%s P%d %s' % (tag, V.degree, name)
                if form.rank == 2:
                    e = _err(assemble(form).to_scipy(), faref.matrix(form), what)
                else:
                    e = _err(assemble(form).get_local(), faref.vector(form),
                             what)
                assert e < 1e-12


def test_identities_with_the_functionals(hip):
    for tag, mesh, m, ids in _cases():
        dsm = Measure('ds', domain=mesh, subdomain_data=m)
        X = SpatialCoordinate(mesh)
        g = 1.0 + X[0] * X[1]
        for V in _spaces(mesh):
            u, v = TrialFunction(V), TestFunction(V)
            w = _field(V, lambda x, y: numpy.sin(2 * x) + y * y)
            what = '%s P%d ' % (tag, V.degree)
            for name, d in (('ds', ds(mesh)), ('ds(k)', dsm(ids[0])),
                            ('ds(wall)', dsm(ids[1]))):
                one = assemble(v * d).get_local()
                assert _err(one.sum(), assemble(1.0 * d),
                            what + 'sum(v %s) = |%s|' % (name, name)) < 1e-12
                A = assemble(u * v * d).to_scipy()
                assert _err(A.dot(numpy.ones(V.N)), one,
                            what + 'row sums of u v %s' % name) < 1e-12
                b = assemble(g * v * d).get_local()
                assert _err(w.array().dot(b), assemble(g * w * d),
                            what + 'w . (g v %s)' % name) < 1e-12
                C = assemble(g * u * v * d)
                assert _err((C * w).get_local(),
                            assemble(g * w * v * d).get_local(),
                            what + '(c u v %s) w' % name) < 1e-12


def test_sparsity(hip):
    for tag, mesh, m, ids in _cases():
        dsm = Measure('ds', domain=mesh, subdomain_data=m)
        n = FacetNormal(mesh)
        for V in _spaces(mesh):
            u, v = TrialFunction(V), TestFunction(V)
            for d, sel in ((ds(mesh), (None, 'everywhere')),
                           (dsm(ids[0]), (m, ids[0])),
                           (dsm(ids[1]), (m, ids[1]))):
                on = faref.touched_dofs(V, *sel)
                assert on.any() and not on.all()
                b = assemble(dot(grad(v), n) * d).get_local()
                assert (b[~on] == 0.0).all() and (b[on] != 0.0).any()
                A = assemble((u * v + dot(grad(u), n) * v) * d).to_scipy()
                A = A.tocoo()
                off = ~(on[A.row] & on[A.col])
                assert (A.data[off] == 0.0).all()
                assert (A.data[~off] != 0.0).any()
            # an empty selection
            b = assemble(v * dsm(NOTHING)).get_local()
            assert b.shape == (V.N,) and (b == 0.0).all()
            A = assemble(u * v * dsm(NOTHING))
            assert (_vals(A) == 0.0).all()


def test_bits(hip):
    for tag, mesh, m, ids in _cases():
        dsm = Measure('ds', domain=mesh, subdomain_data=m)
        for V in _spaces(mesh):
            u, v = TrialFunction(V), TestFunction(V)
            forms_ = dict(_forms(mesh, V, dsm, ids[0]))
            a_ds, L_ds = forms_['variable matrix'], forms_['variable vector']
            # two calls
            assert numpy.array_equal(_vals(assemble(a_ds)),
                                     _vals(assemble(a_ds)))
            assert numpy.array_equal(assemble(L_ds).get_local(),
                                     assemble(L_ds).get_local())
            # a sum is its parts added in the order written
            a_dx = inner(grad(u), grad(v)) * dx
            L_dx = sin(SpatialCoordinate(mesh)[0]) * v * dx
            got = _vals(assemble(a_dx + a_ds - forms_['Robin lhs']))
            want = (_vals(assemble(a_dx)) + _vals(assemble(a_ds))) \
                - _vals(assemble(forms_['Robin lhs']))
            assert numpy.array_equal(got, want)
            got = assemble(L_ds + L_dx).get_local()
            want = assemble(L_ds).get_local() + assemble(L_dx).get_local()
            assert numpy.array_equal(got, want)
            # dx alone: what it was (the comparison of
            # test_bilinear_forms_gpu.py with the dedicated kernels)
            assert _err(_vals(assemble(u * v * dx)),
                        _vals(fem.assemble_mass(V)),
                        '%s P%d mass' % (tag, V.degree)) < 1e-12
            assert _err(_vals(assemble(a_dx)),
                        _vals(fem.assemble_stiffness(V)),
                        '%s P%d stiffness' % (tag, V.degree)) < 1e-12
    # re-marking re-selects: the map follows the markers' version
    tag, mesh, m, ids = _cases()[0]
    dsm = Measure('ds', domain=mesh, subdomain_data=m)
    V = fem.FunctionSpace(mesh, 'CG', 1)
    v = TestFunction(V)
    before = assemble(v * dsm(2)).get_local()
    _Side(lambda x: x[1] < 1e-12).mark(m, 2)
    after = assemble(v * dsm(2)).get_local()
    assert _err(after, faref.vector(v * dsm(2)), 're-marked') < 1e-12
    assert after.sum() > before.sum() + 0.9


def _robin_poisson(n, degree, alpha=2.0):
    mesh = fem.UnitSquareMesh(n, n)
    V = fem.FunctionSpace(mesh, 'CG', degree)
    S = 'sin(pi*x[0])*sin(pi*x[1])'
    exact = fem.Expression(S + ' + x[0]*x[1]', degree=5)
    f = fem.Expression('2.0*pi*pi*' + S, degree=5)
    gx = fem.Expression('pi*cos(pi*x[0])*sin(pi*x[1]) + x[1]', degree=5)
    gy = fem.Expression('pi*sin(pi*x[0])*cos(pi*x[1]) + x[0]', degree=5)
    u, v = TrialFunction(V), TestFunction(V)
    nrm = FacetNormal(mesh)
    a = inner(grad(u), grad(v)) * dx + alpha * u * v * ds
    L = f * v * dx + (dot(as_vector([gx, gy]), nrm) + alpha * exact) * v * ds
    return V, a, L, exact


def test_robin_poisson_orders(hip):
    '''-lap u = f with du/dn + alpha u = g on the whole boundary, no
    DirichletBC: L2 orders over n = 8, 16.'''
    for degree, order in ((1, 1.9), (2, 2.9)):
        errs = []
        for n in (8, 16):
            V, a, L, exact = _robin_poisson(n, degree)
            uh = fem.Function(V)
            info = fem.solve(a == L, uh)
            assert info.method == 'cg'
            errs.append(fem.errornorm(exact, uh))
        rate = numpy.log2(errs[0] / errs[1])
        print('Robin Poisson P%d errors %s order %.3f' % (degree, errs, rate))
        assert rate > order


def test_mixed_conditions_against_sparse_lu(hip):
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla
    mesh = fem.UnitSquareMesh(12, 9)
    m = _square_markers(mesh)
    dsm = Measure('ds', domain=mesh, subdomain_data=m)
    X = SpatialCoordinate(mesh)
    for V in _spaces(mesh):
        u, v = TrialFunction(V), TestFunction(V)
        h, uinf, q = fem.Constant(4.0), fem.Constant(0.25), fem.Constant(1.5)
        a = (1.0 + X[0]) * inner(grad(u), grad(v)) * dx + h * u * v * dsm(3)
        L = sin(X[1]) * v * dx + q * v * dsm(2) + h * uinf * v * dsm(3)
        bcs = [fem.DirichletBC(V, fem.Expression('1.0 + x[1]', degree=1),
                               lambda p, on: on and p[0] < 1e-10)]
        uh = fem.Function(V)
        info = fem.solve(a == L, uh, bcs)
        assert info.method == 'cg'
        dofs, g = fem.bcs.collect(bcs, V.N)
        keep = numpy.ones(V.N)
        keep[dofs] = 0.0
        gfull = numpy.zeros(V.N)
        gfull[dofs] = g
        K = sp.diags(keep)
        A0, b0 = faref.matrix(a), faref.vector(L)
        Aref = K.dot(A0).dot(K) + sp.diags(1.0 - keep)
        bref_ = keep * (b0 - A0.dot(gfull)) + gfull
        A, b = fem.assemble_system(a, L, bcs)
        assert _err(A.to_scipy(), Aref, 'P%d system A' % V.degree) < 1e-12
        assert _err(b.get_local(), bref_, 'P%d system b' % V.degree) < 1e-12
        ref = spla.splu(Aref.tocsc()).solve(bref_)
        e = numpy.linalg.norm(uh.array() - ref) / numpy.linalg.norm(ref)
        print('Dirichlet + flux + Robin P%d: %r, rel l2 vs splu %.2e'
              % (V.degree, info, e))
        assert e < 1e-7


def _radiation(V, m):
    mesh = V.mesh()
    dsm = Measure('ds', domain=mesh, subdomain_data=m)
    u = _field(V, lambda x, y: 1.5 + 0.5 * numpy.sin(3.0 * x)
               * numpy.cos(2.0 * y))
    v = TestFunction(V)
    kappa, f = fem.Constant(0.8), fem.Constant(1.0)
    eps, T = fem.Constant(0.3), fem.Constant(1.2)
    F = kappa * dot(grad(u), grad(v)) * dx - f * v * dx \
        + eps * (u**4 - T**4) * v * dsm(2)
    bcs = [fem.DirichletBC(V, 1.0, lambda p, on: on and p[0] < 1e-10)]
    return u, F, bcs


def test_newton_radiation(hip):
    '''kappa grad u . grad v dx - f v dx + eps (u^4 - T^4) v ds(2).

    J w against (F(u + s w) - F(u - s w)) / (2 s), all three assembled on the
    device.  The form is a quartic polynomial in u, so the truncation error
    of the central difference is exactly s^2 / 6 D^3 F(u)[w, w, w] (D^5 F =
    0): entry i is s^2 / 6 * 24 eps int u w^3 phi_i ds, at most 4 s^2 eps
    max|u| max|w|^3 * 2 lmax (lmax the longest boundary edge: int |phi_i| ds
    is at most the length of the two edges at the dof).  The rounding of the
    two residuals is amplified by 1 / (2 s): an entry of F is a sum of at
    most a row's worth of terms of size up to S_i = sum_j |J_ij| |u_j| + |f_i|
    (J from the host evaluator), each carrying a few ulps from the kernel's
    arithmetic, so 100 eps_machine max S / s bounds it with room.  s = 1e-4
    balances the two within two decades.  The measured error is printed.'''
    mesh = fem.UnitSquareMesh(12, 9)
    m = _square_markers(mesh)
    ev = mesh.edges[mesh.bfacets]
    lmax = numpy.hypot(*(mesh.points[ev[:, 1]] - mesh.points[ev[:, 0]]).T).max()
    for V in _spaces(mesh):
        u, F, bcs = _radiation(V, m)
        J = derivative(F, u)
        w = numpy.cos(2.0 * V.layout.dof_coords[:, 0]) \
            * (1.0 + V.layout.dof_coords[:, 1])
        u0 = u.array().copy()
        Jw = assemble(J).to_scipy().dot(w)
        assert _err(assemble(J).to_scipy(), faref.matrix(J),
                    'P%d J against the host evaluator' % V.degree) < 1e-12
        assert _err(assemble(F).get_local(), faref.vector(F),
                    'P%d F against the host evaluator' % V.degree) < 1e-12
        s = 1.0e-4
        u.set_array(u0 + s * w)
        fp = assemble(F).get_local()
        u.set_array(u0 - s * w)
        fm = assemble(F).get_local()
        u.set_array(u0)
        trunc = 4.0 * s * s * 0.3 * numpy.abs(u0).max() \
            * numpy.abs(w).max()**3 * 2.0 * lmax
        Jh = faref.matrix(J)
        S = (abs(Jh).dot(numpy.abs(u0)) + numpy.abs(faref.vector(
            fem.Constant(1.0) * TestFunction(V) * dx))).max()
        bound = trunc + 100.0 * EPS * S / s
        err = numpy.abs((fp - fm) / (2.0 * s) - Jw).max()
        print('P%d |J w - central difference|_max %.3e  bound %.3e '
              '(truncation %.3e)' % (V.degree, err, bound, trunc))
        assert err <= bound
        # the solve, against the host Newton with the reference matrices
        info = fem.solve(F == 0, u, bcs, J=J)
        assert info.converged and info.fused
        assert [j[0] for j in fem.ops.NewtonAssembler(J, F, V).jobs] == [
            'newton', 'facet_matrix', 'vector', 'facet_vector']
        ur, Fr, bcr = _radiation(V, m)
        res, its = faref.host_newton(Fr, ur, bcr, derivative(Fr, ur))
        print('P%d residuals, device: %s' % (V.degree, info.residuals))
        print('P%d residuals, host:   %s' % (V.degree, res))
        assert info.iterations == its
        e = numpy.linalg.norm(u.array() - ur.array()) \
            / numpy.linalg.norm(ur.array())
        print('radiation P%d: %r; rel l2 vs host Newton %.2e'
              % (V.degree, info, e))
        assert e < 1e-7


def test_robin_eigenmodes(hip):
    k, alpha = 3, 2.0
    for degree in (1, 2):
        V = fem.FunctionSpace(fem.UnitSquareMesh(16, 16), 'CG', degree)
        u, v = TrialFunction(V), TestFunction(V)
        a = inner(grad(u), grad(v)) * dx + alpha * u * v * ds
        m = u * v * dx
        r = fem.Eigenmodes(a, m).solve(k, rtol=1e-9, maxit=400)
        assert r.converged.all()
        A, M = faref.matrix(a), bref.matrix(m)
        isbc = numpy.zeros(V.N, dtype=bool)
        want, _ = eref.smallest(A, M, isbc, k + 2)
        lmin = eref.mass_lambda_min(M, isbc)
        X = numpy.stack([device.to_host(x.data).numpy() for x in r.modes],
                        axis=1)
        MX = M.dot(X)
        R = A.dot(X) - MX * r.values[None, :]
        rn = numpy.sqrt((R * R).sum(axis=0))
        xm = numpy.sqrt((X * MX).sum(axis=0))
        radius = rn / (numpy.sqrt(lmin) * xm) + 1e3 * EPS * abs(want[k - 1])
        print('P%d values %s\nreference %s\nradius %s'
              % (degree, r.values, want[:k], radius))
        assert eref.match_once(r.values, want, radius) == list(range(k))
        assert (numpy.abs(r.values - want[:k]) <= radius).all()
        # alpha > 0 and no Dirichlet condition: no zero eigenvalue
        assert r.values[0] - radius[0] > 0.0
