# -*- coding: utf-8 -*-
'''
Forms of test and trial functions on the HIP path (flow_form_matrix,
flow_form_vector, ops.assemble / assemble_system / solve): against the
dedicated kernels (mass, stiffness, lumped mass, the heat operator), against
the numpy evaluator of tests/bilinear_reference.py at the same rules, action
consistency, determinism, and solves (manufactured Poisson orders, scipy's
sparse LU after the same elimination).  Meshes stay small.
'''
import numpy
import pytest

from flow_amd import fem, _hip
from flow_amd.heat import Heat
from flow_amd.fem import (
    TestFunction, TrialFunction, assemble, dx, SpatialCoordinate, as_vector,
    sin, sqrt, dot, inner, grad, lhs, rhs,
    )

import bilinear_reference as bref

pytestmark = pytest.mark.gpu


def _meshes():
    return [fem.UnitSquareMesh(12, 9),
            fem.karman_channel(60, 14, fitted=True),
            fem.karman_channel_graded(lcar=1.0e-2)]


def _field(V, funcs):
    u = fem.Function(V)
    xy = V.layout.dof_coords
    u.set_array(numpy.concatenate([f(xy[:, 0], xy[:, 1]) for f in funcs]))
    return u


def _err(got, ref, what=''):
    '''max entrywise error relative to max|entry| (printed: the measured
    figure is part of the record).'''
    got = got.toarray() if hasattr(got, 'toarray') else numpy.asarray(got)
    ref = ref.toarray() if hasattr(ref, 'toarray') else numpy.asarray(ref)
    e = numpy.abs(got - ref).max() / numpy.abs(ref).max()
    print('%-44s %.2e' % (what, e))
    return e


def _vals(A):
    return A.plane(0).cpu().numpy()


def _spaces(mesh):
    return [fem.FunctionSpace(mesh, 'CG', k) for k in (1, 2)]


def test_against_dedicated_matrices(hip):
    fcp = {'quadrature_rule': 'vertex', 'representation': 'quadrature'}
    for m, mesh in enumerate(_meshes()):
        for V in _spaces(mesh):
            u, v = TrialFunction(V), TestFunction(V)
            tag = 'mesh %d P%d ' % (m, V.degree)
            A = assemble(u * v * dx)
            assert A.kind == 0 and A.layout is V.layout
            assert _err(_vals(A), _vals(fem.assemble_mass(V)),
                        tag + 'mass') < 1e-12
            assert _err(_vals(assemble(inner(grad(u), grad(v)) * dx)),
                        _vals(fem.assemble_stiffness(V)),
                        tag + 'stiffness') < 1e-12
            lumped = fem.ops.assemble_scalar_matrix(V.layout,
                                                    fem.ops.LUMPED_MASS)
            got = assemble(u * v * dx, form_compiler_parameters=fcp)
            assert _err(_vals(got), _vals(lumped), tag + 'lumped mass') < 1e-12
            if V.degree == 2:       # the zero edge rows, reproduced
                d = got.to_scipy().diagonal()
                assert (d[V.layout.edge_dofs] == 0.0).all()


def test_against_heat_operator(hip):
    for m, mesh in enumerate(_meshes()):
        W = fem.VectorFunctionSpace(mesh, 'CG', 2)
        conv = _field(W, [lambda x, y: 1.0 + x * y - y**2,
                          lambda x, y: 0.5 * x**2 - y])
        source = fem.Expression('1.0 + x[0]*x[1] - 2.0*x[1]*x[1]', degree=2)
        kappa, rho, cp = 0.37, 1.3, 2.1
        for V in _spaces(mesh):
            heat = Heat(V, conv, kappa, rho, cp, [], source)
            u, v = TrialFunction(V), TestFunction(V)
            # the semi-discrete right-hand side of the heat equation, F = 0
            F = - fem.Constant(kappa) * dot(grad(u), grad(v / (rho * cp))) * dx \
                - dot(conv, grad(u)) * v * dx + source * v * dx
            tag = 'mesh %d P%d heat ' % (m, V.degree)
            assert _err(_vals(assemble(lhs(F))), _vals(heat.A), tag + 'A') \
                < 1e-12
            assert _err(assemble(rhs(F)).get_local(), heat.b.get_local(),
                        tag + 'b') < 1e-12


def _variable_forms(mesh, V):
    P2 = fem.FunctionSpace(mesh, 'CG', 2)
    W = fem.VectorFunctionSpace(mesh, 'CG', 2)
    th = _field(P2, [lambda x, y: 0.5 + numpy.sin(3 * x) * y])
    w = _field(W, [lambda x, y: 1.0 + x * y, lambda x, y: numpy.cos(2 * y) - x])
    ex = fem.Expression('exp(x[0]) + x[1]*x[1]', degree=2)
    X = SpatialCoordinate(mesh)
    u, v = TrialFunction(V), TestFunction(V)
    D = as_vector([[1.0 + th * th, 0.3 * X[0]], [0.1 * th, 2.0 + X[1]]])
    beta = as_vector([X[1], -X[0] * th])
    a = (dot(D * grad(u), grad(v)) + sin(X[0]) * u * v
         + dot(w, grad(u)) * v + u * dot(beta, grad(v)) + ex * u * v) * dx
    g = as_vector([th, X[1] * th.dx(0)])
    L = (dot(g, grad(v)) + sin(X[0]) * th * v + ex * v) * dx
    return a, L


def test_variable_coefficients_against_host(hip):
    for m, mesh in enumerate(_meshes()):
        for V in _spaces(mesh):
            a, L = _variable_forms(mesh, V)
            tag = 'mesh %d P%d variable ' % (m, V.degree)
            assert _err(assemble(a).to_scipy(), bref.matrix(a),
                        tag + 'matrix') < 1e-12
            assert _err(assemble(L).get_local(), bref.vector(L),
                        tag + 'vector') < 1e-12
    # a sum of parts at their own degrees, one of them overridden
    mesh = fem.UnitSquareMesh(12, 9)
    V = fem.FunctionSpace(mesh, 'CG', 2)
    u, v = TrialFunction(V), TestFunction(V)
    X = SpatialCoordinate(mesh)
    a = u * v * dx - 2.0 * sin(X[1]) * inner(grad(u), grad(v)) * dx(degree=3)
    assert _err(assemble(a).to_scipy(), bref.matrix(a), 'sum of parts') < 1e-12


def test_action_consistency(hip):
    for m, mesh in enumerate(_meshes()):
        W = fem.VectorFunctionSpace(mesh, 'CG', 2)
        w = _field(W, [lambda x, y: 1.0 + x * y, lambda x, y: numpy.cos(2 * y)])
        X = SpatialCoordinate(mesh)
        for V in _spaces(mesh):
            U = _field(V, [lambda x, y: numpy.sin(2 * x) + y * y])
            u, v = TrialFunction(V), TestFunction(V)

            def form(t):
                return ((1.0 + X[0]**2) * dot(grad(t), grad(v))
                        + dot(w, grad(t)) * v + sin(X[1]) * t * v) * dx
            A = assemble(form(u))
            got = (A * U).get_local()
            assert numpy.array_equal(got, (A @ U.vector()).get_local())
            ref = assemble(form(U)).get_local()
            assert _err(got, ref, 'mesh %d P%d action' % (m, V.degree)) < 1e-12


def test_load_vector_matches_projection_path(hip):
    for m, mesh in enumerate(_meshes()):
        P2 = fem.FunctionSpace(mesh, 'CG', 2)
        th = _field(P2, [lambda x, y: 0.5 + numpy.sin(3 * x) * y])
        X = SpatialCoordinate(mesh)
        f = sqrt(th**2 + 1.0) * X[0] + th.dx(1)
        for V in _spaces(mesh):
            got = assemble(f * TestFunction(V) * dx).get_local()
            ref = fem.ops.form_load_vector(f, V).cpu().numpy()
            assert _err(got, ref, 'mesh %d P%d load vector' % (m, V.degree)) \
                < 1e-13


def test_deterministic(hip):
    mesh = fem.karman_channel(60, 14, fitted=True)
    for V in _spaces(mesh):
        a, L = _variable_forms(mesh, V)
        assert numpy.array_equal(_vals(assemble(a)), _vals(assemble(a)))
        assert numpy.array_equal(assemble(L).get_local(),
                                 assemble(L).get_local())


def _poisson(n, degree):
    mesh = fem.UnitSquareMesh(n, n)
    V = fem.FunctionSpace(mesh, 'CG', degree)
    exact = fem.Expression(
        'sin(pi*x[0])*sin(pi*x[1]) + x[0]*x[1]', degree=5)
    f = fem.Expression('2.0*pi*pi*sin(pi*x[0])*sin(pi*x[1])', degree=4)
    u, v = TrialFunction(V), TestFunction(V)
    a = inner(grad(u), grad(v)) * dx
    L = f * v * dx
    bcs = [fem.DirichletBC(V, fem.Expression('x[0]*x[1]', degree=2),
                           'on_boundary')]
    return V, a, L, bcs, exact


def test_poisson_orders(hip):
    for degree, order in ((1, 1.9), (2, 2.9)):
        errs = []
        for n in (8, 16, 32):
            V, a, L, bcs, exact = _poisson(n, degree)
            uh = fem.Function(V)
            info = fem.solve(a == L, uh, bcs)
            assert info.method == 'cg'
            errs.append(fem.errornorm(exact, uh))
        rates = numpy.log2(numpy.array(errs[:-1]) / numpy.array(errs[1:]))
        print('P%d errors %s orders %s' % (degree, errs, rates))
        assert (rates > order).all()


def _splu_solution(a, L, bcs):
    import scipy.sparse.linalg as spla
    A, b = fem.assemble_system(a, L, bcs)
    return spla.splu(A.to_scipy().tocsc()).solve(b.get_local())


def test_solve_against_sparse_lu(hip):
    V, a, L, bcs, _ = _poisson(16, 2)
    uh = fem.Function(V)
    info = fem.solve(a == L, uh, bcs)
    assert info.method == 'cg'
    ref = _splu_solution(a, L, bcs)
    e = numpy.linalg.norm(uh.array() - ref) / numpy.linalg.norm(ref)
    print('Poisson P2, CG + Jacobi vs splu: rel l2 %.2e (%r)' % (e, info))
    assert e < 1e-7
    # non-symmetric: convection, diffusion, reaction
    mesh = V.mesh()
    X = SpatialCoordinate(mesh)
    W = fem.VectorFunctionSpace(mesh, 'CG', 2)
    w = _field(W, [lambda x, y: 2.0 + y, lambda x, y: -1.0 + x * x])
    u, v = TrialFunction(V), TestFunction(V)
    a = (0.05 * inner(grad(u), grad(v)) + dot(w, grad(u)) * v
         + (1.0 + X[0]) * u * v) * dx
    uh = fem.Function(V)
    info = fem.solve(a == L, uh, bcs)
    assert info.method == 'gmres+ilu0'
    ref = _splu_solution(a, L, bcs)
    e = numpy.linalg.norm(uh.array() - ref) / numpy.linalg.norm(ref)
    print('convection-diffusion-reaction P2, GMRES + ILU(0) vs splu: rel l2 '
          '%.2e (%r)' % (e, info))
    assert e < 1e-7
    # chosen methods, tolerances, and the refusals of solve()
    for method in ('bicgstab', 'gmres', 'cg'):
        uh2 = fem.Function(V)
        prm = {'linear_solver': method,
               'krylov_solver': {'relative_tolerance': 1e-10}}
        if method == 'cg':
            a2, ref2 = inner(grad(u), grad(v)) * dx, None
            ref2 = _splu_solution(a2, L, bcs)
            prm['symmetric'] = True
        else:
            a2, ref2 = a, ref
        info = fem.solve(a2 == L, uh2, bcs, solver_parameters=prm)
        assert info.method.startswith(method)
        assert numpy.linalg.norm(uh2.array() - ref2) \
            < 1e-7 * numpy.linalg.norm(ref2)
    with pytest.raises(_hip.NotConverged):
        fem.solve(a == L, fem.Function(V), bcs, solver_parameters={
            'krylov_solver': {'maximum_iterations': 1}})
    assert issubclass(_hip.NotConverged, RuntimeError)
    for direct in ('lu', 'mumps', 'umfpack'):
        with pytest.raises(ValueError, match='no direct solver'):
            fem.solve(a == L, uh, bcs,
                      solver_parameters={'linear_solver': direct})


def test_assemble_system_and_apply(hip):
    import scipy.sparse as sp
    V, a, L, bcs, _ = _poisson(9, 2)
    mesh = V.mesh()
    u, v = TrialFunction(V), TestFunction(V)
    a = a + dot(as_vector([1.0, 2.0]), grad(u)) * v * dx
    A0 = assemble(a).to_scipy()
    b0 = assemble(L).get_local()
    dofs, g = fem.bcs.collect(bcs, V.N)
    A, b = fem.assemble_system(a, L, bcs)
    keep = numpy.ones(V.N)
    keep[dofs] = 0.0
    gfull = numpy.zeros(V.N)
    gfull[dofs] = g
    K = sp.diags(keep)
    Aref = K.dot(A0).dot(K) + sp.diags(1.0 - keep)
    bref_ = keep * (b0 - A0.dot(gfull)) + gfull
    assert _err(A.to_scipy(), Aref, 'assemble_system A') < 1e-12
    assert _err(b.get_local(), bref_, 'assemble_system b') < 1e-12
    # L = None: a zero right-hand side, lifted
    _, bz = fem.assemble_system(a, None, bcs)
    assert _err(bz.get_local(), keep * (-A0.dot(gfull)) + gfull,
                'assemble_system b, L = None') < 1e-12
    # without conditions: the plain pair
    A1, b1 = fem.assemble_system(a, L)
    assert numpy.array_equal(_vals(A1), _vals(assemble(a)))
    assert numpy.array_equal(b1.get_local(), b0)
    # identity rows: rows replaced, columns kept
    A2, b2 = assemble(a), assemble(L)
    bcs[0].apply(A2, b2)
    Aid = K.dot(A0) + sp.diags(1.0 - keep)
    assert _err(A2.to_scipy(), Aid, 'bc.apply(A, b): A') < 1e-15
    assert numpy.array_equal(b2.get_local(), keep * b0 + gfull)
    A3, b3 = assemble(a), assemble(L)
    bcs[0].apply(A3)
    bcs[0].apply(b3)
    assert numpy.array_equal(_vals(A3), _vals(A2))
    assert numpy.array_equal(b3.get_local(), b2.get_local())
    del mesh


def test_refusals_with_the_library(hip):
    mesh = fem.UnitSquareMesh(4, 4)
    V1, V2 = _spaces(mesh)
    u, v = TrialFunction(V1), TestFunction(V1)
    a, L = u * v * dx, fem.Constant(1.0) * v * dx
    with pytest.raises(ValueError, match='ranks'):
        assemble(a + L)
    with pytest.raises(NotImplementedError, match='different spaces'):
        fem.assemble_system(a, fem.Constant(1.0) * TestFunction(V2) * dx)
    with pytest.raises(ValueError, match='another space'):
        fem.assemble_system(a, L, [fem.DirichletBC(V2, 0.0, 'on_boundary')])
    with pytest.raises(ValueError, match='bilinear'):
        fem.solve(L == L, fem.Function(V1))
    with pytest.raises(ValueError, match='space of the trial'):
        fem.solve(a == L, fem.Function(V2))
    with pytest.raises(TypeError):
        fem.solve(a, fem.Function(V1))
    with pytest.raises(ValueError, match='different meshes'):
        assemble(u * v * dx(fem.UnitSquareMesh(2, 2)))
    # the C entry points refuse malformed programs (check_form); the
    # messages are matched whole: 'invalid argument: <rule> (<condition>)'
    from flow_amd.fem import forms, ops
    import ctypes
    lib = _hip.lib()
    buf = ops.scratch(mesh, 9 * mesh.num_cells())
    out = ops.value_plane(V1.layout)
    vec = fem.Function(V1).data

    def call(fs, matrix=True):
        fn = lib.flow_form_matrix if matrix else lib.flow_form_vector
        _hip.check(fn(
            ctypes.byref(ops.mesh_struct(mesh)),
            ctypes.byref(ops.space_struct(V1.layout)), ctypes.byref(fs),
            _hip.f64(buf), _hip.f64(out if matrix else vec), _hip.stream()))

    def struct(prog):
        return ops._form_struct(prog, mesh, 2)

    one = ('num', 1.0)
    # a one-output program where a 9- or 3-slot table is expected
    fs, keep = struct(forms.Program([one]))
    with pytest.raises(ValueError, match=r'^invalid argument: form outputs \('):
        call(fs)
    with pytest.raises(ValueError, match=r'^invalid argument: form outputs \('):
        call(fs, matrix=False)
    # a slot out of range (instruction 1 is the `out`)
    for nout, matrix in ((9, True), (3, False)):
        fs, keep = struct(forms.Program([one], slots=[0], nout=nout))
        assert fs.prog[4] == forms.OPS['out']
        fs.prog[4 + 3] = nout
        with pytest.raises(ValueError,
                           match=r'^invalid argument: form output \('):
            call(fs, matrix)
    # one slot written twice
    fs, keep = struct(forms.Program([one, one], slots=[4, 4], nout=9))
    with pytest.raises(
            ValueError,
            match=r'^invalid argument: form output slot written twice \('):
        call(fs)
    # no slot written at all: the `out` turned into a `mov`
    fs, keep = struct(forms.Program([one], slots=[0], nout=9))
    fs.prog[4] = forms.OPS['mov']
    with pytest.raises(
            ValueError,
            match=r'^invalid argument: form writes no coefficient slot \('):
        call(fs)
    # the facet normal is refused
    fs, keep = struct(forms.Program([('n', 0)], facet=True, slots=[0], nout=9))
    with pytest.raises(ValueError, match=r'^invalid argument: form opcode \('):
        call(fs)
    # ... and a well-formed table goes through
    fs, keep = struct(forms.Program([one], slots=[0], nout=9))
    call(fs)
    M = fem.assemble_mass(V1)
    assert _err(out[:V1.layout.nnz].cpu().numpy(), _vals(M),
                'hand-made mass table') < 1e-12
    del keep
