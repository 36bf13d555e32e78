# -*- coding: utf-8 -*-
'''
Forms of test and trial functions on vector spaces on the HIP path
(flow_form_block_matrix, flow_form_block_vector, flow_bc_symmetric_blocks):
blocks bitwise against the scalar forms, matrices and vectors against the
host evaluator of tests/vector_form_reference.py, operator consistency,
determinism, Dirichlet elimination against scipy, and solves (manufactured
elasticity with a traction side, a non-symmetric Brinkman operator).
'''
import numpy
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from flow_amd import fem, _hip
from flow_amd.fem import (
    TestFunction, TrialFunction, assemble, dx, Measure, MeshFunction,
    SpatialCoordinate, as_vector, sin, cos, dot, inner, grad, div, sym, tr,
    Identity, outer,
    )

import vector_form_reference as vref
from form_assembly_cases import long_integrands

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _switches_on():
    '''Vector arguments (and those under ds) are off by default: on for these
    tests only.'''
    with fem.vector_arguments(True), fem.facet_arguments(True):
        yield


class _Side(fem.SubDomain):
    def __init__(self, test):
        fem.SubDomain.__init__(self)
        self.test = test

    def inside(self, x, on_boundary):
        return on_boundary & self.test(x)


def _meshes():
    return [fem.UnitSquareMesh(12, 9), fem.karman_channel(60, 14, fitted=True)]


def _pairs(mesh):
    return [(fem.VectorFunctionSpace(mesh, 'CG', k),
             fem.FunctionSpace(mesh, 'CG', k)) for k in (1, 2)]


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
    print('%-52s %.2e' % (what, e))
    return e


def _plane(A, p):
    return A.plane(p).cpu().numpy()


def _eps(w):
    return sym(grad(w))


def _sigma(w, mu, lam):
    return 2.0 * mu * _eps(w) + lam * tr(_eps(w)) * Identity(2)


def test_diagonal_blocks_bitwise(hip):
    for m, mesh in enumerate(_meshes()):
        for W, V in _pairs(mesh):
            u, v = TrialFunction(W), TestFunction(W)
            us, vs = TrialFunction(V), TestFunction(V)
            for name, a, a_s in (
                    ('Laplacian', inner(grad(u), grad(v)) * dx,
                     inner(grad(us), grad(vs)) * dx),
                    ('mass', dot(u, v) * dx, us * vs * dx)):
                A = assemble(a)
                assert A.kind == 2 and A.size == 2 * W.N
                ref = _plane(assemble(a_s), 0)
                assert numpy.abs(ref).max() > 0.0
                for p in (0, 3):
                    assert numpy.array_equal(_plane(A, p), ref), (m, name, p)
                for p in (1, 2):
                    assert not _plane(A, p).any(), (m, name, p)
                assert numpy.array_equal(A.vals.cpu().numpy(),
                                         assemble(a).vals.cpu().numpy())
            # rank 1: the components of a load are the scalar loads
            f = fem.Expression(('sin(x[0])*x[1]', '1.0 + x[0]'), degree=3)
            b = assemble(dot(f, v) * dx).get_local()
            assert b.shape == (2 * W.N,)
            for r in range(2):
                assert numpy.array_equal(
                    b[r * W.N:(r + 1) * W.N],
                    assemble(f[r] * vs * dx).get_local())
            one = assemble(v[1] * dx).get_local()
            assert not one[:W.N].any() and one[W.N:].any()


def _variable_forms(mesh, W):
    '''A variable-coefficient pair: a field-dependent tensor, a sin(x)
    reaction, both orientations of a first-order term, an Expression.'''
    X = SpatialCoordinate(mesh)
    w = _field(W, [lambda x, y: 1.0 + x * y, lambda x, y: y - 0.5 * x * x])
    k = fem.Expression('1.0 + x[0]*x[0] + 0.5*x[1]', degree=2)
    K = Identity(2) + outer(w, w)
    u, v = TrialFunction(W), TestFunction(W)
    a = (inner(dot(grad(u), K), grad(v)) + (2.0 + sin(X[0])) * dot(u, v)
         + dot(dot(grad(u), w), v) + dot(u, dot(grad(v), w))
         + k * div(u) * div(v) + k * u[0] * v[1]) * dx
    g = fem.Expression(('cos(x[1])', 'x[0]*x[1]'), degree=3)
    L = (dot(g, v) + inner(outer(w, X), grad(v)) + k * dot(w, w) * v[0]
         + sin(X[1]) * div(v)) * dx
    return a, L


def test_against_host_evaluator(hip):
    mu, lam = fem.Constant(1.3), fem.Constant(0.7)
    for m, mesh in enumerate(_meshes()):
        for W, _ in _pairs(mesh):
            tag = 'mesh %d P%d ' % (m, W.degree)
            u, v = TrialFunction(W), TestFunction(W)
            a = inner(_sigma(u, mu, lam), _eps(v)) * dx
            A = assemble(a)
            S = A.to_scipy()
            assert _err(S, vref.matrix(a), tag + 'elasticity') < 1e-12
            assert _err(S, S.T, tag + 'elasticity symmetry') < 1e-14
            assert numpy.array_equal(A.vals.cpu().numpy(),
                                     assemble(a).vals.cpu().numpy())
            a, L = _variable_forms(mesh, W)
            A, b = assemble(a), assemble(L)
            assert _err(A.to_scipy(), vref.matrix(a), tag + 'variable a') \
                < 1e-12
            assert _err(b.get_local(), vref.vector(L), tag + 'variable L') \
                < 1e-12
            assert numpy.array_equal(A.vals.cpu().numpy(),
                                     assemble(a).vals.cpu().numpy())
            assert numpy.array_equal(b.get_local(), assemble(L).get_local())
            # a sum of parts, added in the order written
            s = a - 0.5 * inner(grad(u), grad(v)) * dx + dot(u, v) * dx
            assert _err(assemble(s).to_scipy(), vref.matrix(s),
                        tag + 'sum of parts') < 1e-12


def test_action_consistency(hip):
    mu, lam = fem.Constant(1.3), fem.Constant(0.7)
    for m, mesh in enumerate(_meshes()):
        for W, _ in _pairs(mesh):
            U = _field(W, [lambda x, y: numpy.sin(2.0 * x) + y,
                           lambda x, y: x * y - numpy.cos(y)])
            u, v = TrialFunction(W), TestFunction(W)
            w = _field(W, [lambda x, y: 1.0 + y, lambda x, y: -x])
            a = (inner(_sigma(u, mu, lam), _eps(v))
                 + dot(dot(grad(u), w), v) + 3.0 * dot(u, v)) * dx
            action = (inner(_sigma(U, mu, lam), _eps(v))
                      + dot(dot(grad(U), w), v) + 3.0 * dot(U, v)) * dx
            got = (assemble(a) * U).get_local()
            ref = assemble(action).get_local()
            assert _err(got, ref, 'mesh %d P%d A*U vs action'
                        % (m, W.degree)) < 1e-12


def test_blocks_of_several_programs(hip):
    """The further programs of a block: the spare scratch plane and
    plane_add_kernel under dx, the zeroed plane and the sum under ds."""
    from flow_amd.fem import forms
    mesh = fem.UnitSquareMesh(12, 9)
    dsm = Measure('ds', domain=mesh, subdomain_data=_square_markers(mesh))
    for W, _ in _pairs(mesh):
        ia, iL = long_integrands(mesh, W)
        for name, form, rank in (('dx matrix', ia * dx, 2),
                                 ('dx vector', iL * dx, 1),
                                 ('ds matrix', ia * dsm(2), 2),
                                 ('ds vector', iL * dsm(2), 1),
                                 ('dx + ds matrix', ia * dx + ia * dsm(3), 2)):
            tag = 'P%d several programs, %s' % (W.degree, name)
            part = form.terms()[0][1]
            _, table = part.argument_table()
            counts = dict(
                (p, len(forms.argument_programs(
                    block, rank, part.integral_type != 'cell')))
                for p, block in forms.block_items(table, rank))
            assert counts[0] >= 3 and min(counts.values()) == 1, counts
            got = assemble(form)
            again = assemble(form)
            if rank == 2:
                assert _err(got.to_scipy(), vref.matrix(form), tag) < 1e-12
                assert numpy.array_equal(got.vals.cpu().numpy(),
                                         again.vals.cpu().numpy())
            else:
                assert _err(got.get_local(), vref.vector(form), tag) < 1e-12
                assert numpy.array_equal(got.get_local(), again.get_local())


def _square_markers(mesh):
    '''1 left, 2 right, 3 top; the bottom stays 0.'''
    m = MeshFunction('size_t', mesh, 1, 0)
    _Side(lambda x: x[0] < 1e-12).mark(m, 1)
    _Side(lambda x: x[0] > 1.0 - 1e-12).mark(m, 2)
    _Side(lambda x: x[1] > 1.0 - 1e-12).mark(m, 3)
    return m


def test_facet_parts(hip):
    mesh = fem.UnitSquareMesh(12, 9)
    dsm = Measure('ds', domain=mesh, subdomain_data=_square_markers(mesh))
    X = SpatialCoordinate(mesh)
    for W, _ in _pairs(mesh):
        tag = 'P%d ' % W.degree
        u, v = TrialFunction(W), TestFunction(W)
        t = fem.Expression(('1.0 + x[1]', 'sin(x[0])'), degree=3)
        h = 2.0 + X[0] * X[1]
        for k in (2, 3):
            L = dot(t, v) * dsm(k)
            a = h * dot(u, v) * dsm(k)
            bk = assemble(L).get_local()
            assert _err(bk, vref.vector(L), tag + 'traction ds(%d)' % k) \
                < 1e-12
            Ak = assemble(a)
            assert _err(Ak.to_scipy(), vref.matrix(a),
                        tag + 'Robin ds(%d)' % k) < 1e-12
            assert numpy.array_equal(bk, assemble(L).get_local())
            assert numpy.array_equal(Ak.vals.cpu().numpy(),
                                     assemble(a).vals.cpu().numpy())
        # with cell parts, a mixed block under ds, every facet, and nothing
        a = (inner(grad(u), grad(v)) * dx + h * dot(u, v) * dsm(2)
             + u[0] * v[1] * dsm + dot(u, v) * dsm(99))
        assert _err(assemble(a).to_scipy(), vref.matrix(a), tag + 'dx + ds') \
            < 1e-12
        L = dot(t, v) * dx - dot(t, v) * dsm(3) + v[1] * dsm(99)
        assert _err(assemble(L).get_local(), vref.vector(L),
                    tag + 'dx - ds') < 1e-12


def _eliminated(A0, b0, dofs, g):
    n = A0.shape[0]
    keep = numpy.ones(n)
    keep[dofs] = 0.0
    gfull = numpy.zeros(n)
    gfull[dofs] = g
    K = sp.diags(keep)
    return (K.dot(A0).dot(K) + sp.diags(1.0 - keep),
            keep * (b0 - A0.dot(gfull)) + gfull, K, keep, gfull)


def test_assemble_system_and_apply(hip):
    mesh = fem.UnitSquareMesh(12, 9)
    mu, lam = fem.Constant(1.3), fem.Constant(0.7)
    left = _Side(lambda x: x[0] < 1e-12)
    top = _Side(lambda x: x[1] > 1.0 - 1e-12)
    for W, _ in _pairs(mesh):
        u, v = TrialFunction(W), TestFunction(W)
        w = _field(W, [lambda x, y: 1.0 + y, lambda x, y: -x])
        a = (inner(_sigma(u, mu, lam), _eps(v))
             + dot(dot(grad(u), w), v)) * dx
        L = dot(fem.Expression(('x[1]', '1.0 - x[0]'), degree=1), v) * dx
        A0 = assemble(a).to_scipy()
        b0 = assemble(L).get_local()
        gW = fem.Expression(('x[0] + x[1]', 'x[0]*x[1] - 1.0'), degree=2)
        cases = (
            ('W', [fem.DirichletBC(W, gW, 'on_boundary')]),
            ('W.sub(0)', [fem.DirichletBC(W.sub(0), 0.25, left)]),
            ('both', [fem.DirichletBC(W.sub(0), fem.Expression(
                'x[1]', degree=1), left),
                fem.DirichletBC(W.sub(1), -1.5, top)]))
        for name, bcs in cases:
            tag = 'P%d %s: ' % (W.degree, name)
            dofs, g = fem.bcs.collect(bcs, W.size())
            assert len(dofs) > 0
            if name == 'W.sub(0)':
                assert dofs.max() < W.N
            if name == 'both':
                assert dofs.min() < W.N <= dofs.max()
            Aref, bref_, K, keep, gfull = _eliminated(A0, b0, dofs, g)
            A, b = fem.assemble_system(a, L, bcs)
            assert A.kind == 2
            assert _err(A.to_scipy(), Aref, tag + 'assemble_system A') < 1e-12
            assert _err(b.get_local(), bref_, tag + 'assemble_system b') \
                < 1e-12
            A_, b_ = fem.assemble_system(a, L, bcs)
            assert numpy.array_equal(A.vals.cpu().numpy(),
                                     A_.vals.cpu().numpy())
            assert numpy.array_equal(b.get_local(), b_.get_local())
            _, bz = fem.assemble_system(a, None, bcs)
            assert _err(bz.get_local(), keep * (-A0.dot(gfull)) + gfull,
                        tag + 'L = None') < 1e-12
            # identity rows: rows replaced, columns kept
            A2, b2 = assemble(a), assemble(L)
            for bc in bcs:
                bc.apply(A2, b2)
            Aid = K.dot(A0) + sp.diags(1.0 - keep)
            assert _err(A2.to_scipy(), Aid, tag + 'bc.apply(A, b): A') < 1e-15
            assert numpy.array_equal(b2.get_local(), keep * b0 + gfull)
        A1, b1 = fem.assemble_system(a, L)
        assert numpy.array_equal(A1.vals.cpu().numpy(),
                                 assemble(a).vals.cpu().numpy())
        assert numpy.array_equal(b1.get_local(), b0)
        V = fem.FunctionSpace(mesh, 'CG', W.degree)
        with pytest.raises(ValueError, match='another space'):
            fem.assemble_system(a, L, [fem.DirichletBC(V, 0.0, left)])


MU, LAM = 1.0, 1.5


def _elasticity(n, degree):
    '''-div sigma(u) = f on the unit square; u given on the left, bottom and
    top sides, the traction sigma(u) n on the right side (through ds).'''
    mesh = fem.UnitSquareMesh(n, n)
    W = fem.VectorFunctionSpace(mesh, 'CG', degree)
    exact = fem.Expression(('sin(x[0])*cos(x[1])', 'x[0]*x[0]*x[1]'),
                           degree=5)
    f = fem.Expression(
        ('%r*sin(x[0])*cos(x[1]) - %r*x[0]' % (3 * MU + LAM, 2 * (LAM + MU)),
         '%r*cos(x[0])*sin(x[1]) - %r*x[1]' % (MU + LAM, 2 * MU)), degree=4)
    t = fem.Expression(
        ('%r*cos(x[0])*cos(x[1]) + %r*x[0]*x[0]' % (2 * MU + LAM, LAM),
         '%r*(2.0*x[0]*x[1] - sin(x[0])*sin(x[1]))' % MU), degree=4)
    m = MeshFunction('size_t', mesh, 1, 0)
    _Side(lambda x: x[0] > 1.0 - 1e-12).mark(m, 2)
    dsm = Measure('ds', domain=mesh, subdomain_data=m)
    u, v = TrialFunction(W), TestFunction(W)
    F = inner(_sigma(u, fem.Constant(MU), fem.Constant(LAM)), _eps(v)) * dx \
        - dot(f, v) * dx - dot(t, v) * dsm(2)
    a, L = fem.system(F)
    bcs = [fem.DirichletBC(W, exact, _Side(
        lambda x: (x[0] < 1e-12) | (x[1] < 1e-12) | (x[1] > 1.0 - 1e-12)))]
    return W, a, L, bcs, exact


def _splu_solution(a, L, bcs):
    A, b = fem.assemble_system(a, L, bcs)
    return spla.splu(A.to_scipy().tocsc()).solve(b.get_local())


def test_elasticity_orders(hip):
    for degree, order in ((1, 1.9), (2, 2.9)):
        errs, its = [], []
        for n in (8, 16, 32):
            W, a, L, bcs, exact = _elasticity(n, degree)
            uh = fem.Function(W)
            info = fem.solve(a == L, uh, bcs)
            assert info.method == 'cg'
            its.append(info.iterations)
            errs.append(fem.errornorm(exact, uh))
        rates = numpy.log2(numpy.array(errs[:-1]) / numpy.array(errs[1:]))
        print('P%d errors %s orders %s CG iterations %s'
              % (degree, errs, rates, its))
        assert (rates > order).all()


def test_solves_against_sparse_lu(hip):
    W, a, L, bcs, _ = _elasticity(16, 2)
    uh = fem.Function(W)
    info = fem.solve(a == L, uh, bcs)
    assert info.method == 'cg'
    ref = _splu_solution(a, L, bcs)
    e = numpy.linalg.norm(uh.array() - ref) / numpy.linalg.norm(ref)
    print('elasticity P2, CG + Jacobi vs splu: rel l2 %.2e (%r)' % (e, info))
    assert e < 1e-7
    # non-symmetric: a Brinkman / penalised momentum operator
    mesh = W.mesh()
    w = _field(W, [lambda x, y: 2.0 + y, lambda x, y: -1.0 + x * x])
    u, v = TrialFunction(W), TestFunction(W)
    a = 0.05 * inner(grad(u), grad(v)) * dx \
        + (dot(dot(grad(u), w), v) + 4.0 * dot(u, v)) * dx
    uh = fem.Function(W)
    info = fem.solve(a == L, uh, bcs)
    assert info.method == 'gmres+ilu0'
    ref = _splu_solution(a, L, bcs)
    e = numpy.linalg.norm(uh.array() - ref) / numpy.linalg.norm(ref)
    print('Brinkman P2, GMRES + ILU(0) vs splu: rel l2 %.2e (%r)' % (e, info))
    assert e < 1e-7
    with pytest.raises(_hip.NotConverged):
        fem.solve(a == L, fem.Function(W), bcs, solver_parameters={
            'krylov_solver': {'maximum_iterations': 1}})
    V = fem.FunctionSpace(mesh, 'CG', 2)
    with pytest.raises(ValueError, match='space of the trial function'):
        fem.solve(a == L, fem.Function(V), bcs)


def test_refusals_of_the_entry_points(hip):
    '''flow_form_block_matrix / _vector and flow_bc_symmetric_blocks check
    their arguments before anything is launched: strips, the block tag, the
    programs (check_form), distinct in and out planes.'''
    import ctypes
    from flow_amd.fem import forms, ops
    lib = _hip.lib()
    mesh = fem.UnitSquareMesh(4, 4)
    W = fem.VectorFunctionSpace(mesh, 'CG', 1)
    lay = W.layout
    nc = mesh.num_cells()
    one = ('num', 1.0)
    stride = ops.plane_stride(lay)
    buf = ops.scratch(mesh, 4 * 9 * nc)
    vals = ops.Matrix(lay, 2).vals
    vec = fem.Function(W).data

    def call(progs, tags, matrix=True, ms=None, ss=None):
        structs = (_hip.FormS * len(progs))()
        keeps = []
        for k, prog in enumerate(progs):
            structs[k], keep = ops._form_struct(prog, mesh, 2)
            keeps.append(keep)
        ctags = (ctypes.c_int * len(tags))(*tags)
        ms = ops.mesh_struct(mesh) if ms is None else ms
        ss = ops.space_struct(lay) if ss is None else ss
        if matrix:
            rc = lib.flow_form_block_matrix(
                ctypes.byref(ms), ctypes.byref(ss), len(progs), structs,
                ctags, _hip.f64(buf), _hip.f64(vals), stride, _hip.stream())
        else:
            rc = lib.flow_form_block_vector(
                ctypes.byref(ms), ctypes.byref(ss), len(progs), structs,
                ctags, _hip.f64(buf), _hip.f64(vec), _hip.stream())
        _hip.check(rc)

    mass = forms.Program([one], slots=[0], nout=9)
    load = forms.Program([one], slots=[0], nout=3)
    strip = _hip.MeshS.from_buffer_copy(ops.mesh_struct(mesh))
    strip.c0, strip.c1 = 0, nc // 2
    rows = _hip.SpaceS.from_buffer_copy(ops.space_struct(lay))
    rows.r0, rows.r1 = 0, lay.N // 2
    for matrix, prog in ((True, mass), (False, load)):
        for kw in ({'ms': strip}, {'ss': rows}):
            with pytest.raises(ValueError, match='on strips'):
                call([prog], [0], matrix, **kw)
        for tag in (-1, 4 if matrix else 2):
            with pytest.raises(ValueError, match='block tag'):
                call([prog], [tag], matrix)
        with pytest.raises(ValueError, match='form outputs'):
            call([load if matrix else mass], [0], matrix)
        with pytest.raises(ValueError, match='block programs'):
            call([], [], matrix)
    # ... and well-formed calls go through: two mass blocks, block 3 twice
    call([mass, mass, mass], [0, 3, 3])
    A = ops.Matrix(lay, 2, vals)
    V = fem.FunctionSpace(mesh, 'CG', 1)
    M = assemble(TrialFunction(V) * TestFunction(V) * dx).plane(0)
    assert numpy.array_equal(_plane(A, 0), M.cpu().numpy())
    assert numpy.array_equal(_plane(A, 3), (M + M).cpu().numpy())
    assert not _plane(A, 1).any() and not _plane(A, 2).any()
    import torch
    mask = ops.device.zeros(2 * lay.N, dtype=torch.uint8)
    with pytest.raises(ValueError, match='distinct buffers'):
        _hip.check(lib.flow_bc_symmetric_blocks(
            lay.N, lay.nnz, _hip.i32(lay.dev('rowptr')),
            _hip.i32(lay.dev('cols')), _hip.f64(vals), stride,
            _hip.u8(mask), _hip.f64(vals), stride, _hip.stream()))
