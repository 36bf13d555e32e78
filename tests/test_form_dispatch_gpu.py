# -*- coding: utf-8 -*-
'''
The launch dispatcher of csrc/form_kernels.hip: every (number of fields,
extended) arm of every form entry point reaches its own kernel instance.  The
other suites use one to three fields; an arm that launched the instance of
another field count would read outside the fields the lane holds or drop
some.

Per entry point and k = 0..6 fields the coefficient is c0 + sum_j w_j f_j with
distinct weights and distinct positive affine fields f_j (P1 and P2 in turn):
a dropped or swapped field changes the result.  Each case runs twice: as it
is, and as max_value(coefficient, -1), the identity on positive values, which
puts an extended opcode into the program and so selects the EXT instance.  The
expected values come from the numpy references of the suite of that entry
point, at that suite's tolerance, evaluated for the plain coefficient (the
references of the cell forms do not know max_value, and the value is the
same).  Every program the front end compiles on the way is checked to hold k
fields and to be extended exactly where the case means it: otherwise the test
could pass without visiting the arm.

flow_form_newton: the state u is a field of the fused program itself, so the
front end reaches its arms 1..6 only (k - 1 coefficient fields and u).

A 2 x 2 unit square (8 cells), P1 and P2 where the entry point has a degree.
'''
import numpy
import pytest

from flow_amd import device, fem
from flow_amd.fem import (
    TestFunction, TrialFunction, assemble, dx, ds, derivative, max_value, dot,
    as_vector, forms, ops,
    )

import bilinear_reference as bref
import facet_argument_reference as faref
import facet_reference as fac
import form_reference as fref
import point_reference as pointref
import profile_reference as pref
import vector_form_reference as vref

pytestmark = pytest.mark.gpu

C0 = 0.7
WEIGHTS = (1.3, -0.4, 2.1, 0.6, -1.7, 0.9)
# f_j = a + b x + c y > 0.4 on the unit square; C0 + sum of any first k of
# WEIGHTS[j] f_j stays above -1
AFFINE = ((1.0, 0.5, 0.25), (0.5, 0.2, 0.6), (2.0, -0.7, 0.3),
          (0.8, 0.4, -0.3), (0.6, 0.1, 0.05), (1.5, -0.5, -0.5))
POINTS = numpy.array([[0.1, 0.2], [0.6, 0.3], [0.35, 0.8], [0.9, 0.95],
                      [0.5, 0.5]])


@pytest.fixture(autouse=True)
def _facet_arguments_on():
    with fem.facet_arguments(True):
        yield


@pytest.fixture(scope='module')
def case():
    mesh = fem.UnitSquareMesh(2, 2)
    assert mesh.num_cells() == 8
    spaces = {k: fem.FunctionSpace(mesh, 'CG', k) for k in (1, 2)}
    fields = []
    for j, (a, b, c) in enumerate(AFFINE):
        V = spaces[1 + j % 2]
        f = fem.Function(V)
        xy = V.layout.dof_coords
        f.set_array(a + b * xy[:, 0] + c * xy[:, 1])
        assert f.array().min() > 0.4
        fields.append(f)
    return mesh, spaces, fields


@pytest.fixture
def programs(monkeypatch):
    '''(fields, extended) of every program handed to the library.'''
    seen = []
    inner = ops._form_struct

    def spy(prog, *args, **kwargs):
        seen.append((len(prog.fields),
                     any(ins[0] >= forms.OPS['lt'] for ins in prog.code)))
        return inner(prog, *args, **kwargs)

    monkeypatch.setattr(ops, '_form_struct', spy)
    return seen


def _coefficient(fields, k, ext):
    co = forms.as_form(fem.Constant(C0))
    for j in range(k):
        co = co + WEIGHTS[j] * fields[j]
    return max_value(co, -1.0) if ext else co


def _cases(lo=0):
    return [(k, ext) for k in range(lo, 7) for ext in (False, True)]


def _visited(programs, k, ext):
    '''Every program since the last call held k fields and the flag.'''
    assert programs and set(programs) == {(k, ext)}, (programs, k, ext)
    del programs[:]


def _rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


def _err(got, ref):
    got = got.toarray() if hasattr(got, 'toarray') else numpy.asarray(got)
    ref = ref.toarray() if hasattr(ref, 'toarray') else numpy.asarray(ref)
    return numpy.abs(got - ref).max() / numpy.abs(ref).max()


def test_functional_and_load_vector(hip, case, programs):
    '''tests/test_forms_gpu.py: 1e-12 relative; entries 1e-12 of the largest.'''
    mesh, spaces, fields = case
    for k, ext in _cases():
        plain = _coefficient(fields, k, False)
        co = _coefficient(fields, k, ext)
        assert _rel(assemble(co * dx(mesh)), fref.functional(plain * dx(mesh))) < 1e-12
        _visited(programs, k, ext)
        for V in spaces.values():
            b = ops.form_load_vector(co, V).cpu().numpy()
            ref = fref.load_vector(plain, V)
            assert numpy.abs(b - ref).max() < 1e-12 * numpy.abs(ref).max(), (k, ext)
            _visited(programs, k, ext)


def test_facet_functional(hip, case, programs):
    '''tests/test_facet_forms_gpu.py: 1e-12 of max(int |f|, the length).'''
    mesh, spaces, fields = case
    for k, ext in _cases():
        plain = _coefficient(fields, k, False)
        got = assemble(_coefficient(fields, k, ext) * ds(mesh))
        _visited(programs, k, ext)
        want = fac.functional(plain * ds(mesh))
        scale = max(fac.functional(abs(plain) * ds(mesh)),
                    fac.functional(1.0 * ds(mesh)))
        assert abs(got - want) <= 1e-12 * scale, (k, ext, got, want)


def test_facet_values(hip, case, programs):
    '''tests/test_profile_gpu.py: 1e-12 of the largest sample.'''
    mesh, spaces, fields = case
    P = fem.BoundaryProfile(mesh, degree=2)
    R = pref.Reference(mesh, range(len(mesh.bfacets)), 2)
    for k, ext in _cases():
        got = device.to_host(P.evaluate(_coefficient(fields, k, ext))).numpy()
        _visited(programs, k, ext)
        want = C0 + sum(WEIGHTS[j] * R.field(fields[j]) for j in range(k)) \
            + numpy.zeros(P.npoints)
        assert got.shape == (1, P.npoints)
        assert numpy.abs(got[0] - want).max() < 1e-12 * numpy.abs(want).max(), (k, ext)


def test_points(hip, case, programs):
    '''tests/test_points_gpu.py, against the numpy evaluator: 1e-13 of the
    largest value.'''
    mesh, spaces, fields = case
    probes = fem.Probes(mesh, POINTS)
    assert probes.found.all()
    values = [pointref.field_values(f, POINTS, probes.cells)[0] for f in fields]
    for k, ext in _cases():
        got = probes(_coefficient(fields, k, ext))
        _visited(programs, k, ext)
        want = C0 + sum(WEIGHTS[j] * values[j] for j in range(k)) \
            + numpy.zeros(len(POINTS))
        assert numpy.abs(got - want).max() <= 1e-13 * numpy.abs(want).max(), (k, ext)


def test_matrix_and_vector(hip, case, programs):
    '''tests/test_bilinear_forms_gpu.py: entries 1e-12 of the largest.'''
    mesh, spaces, fields = case
    for V in spaces.values():
        u, v = TrialFunction(V), TestFunction(V)
        for k, ext in _cases():
            plain = _coefficient(fields, k, False)
            co = _coefficient(fields, k, ext)
            assert _err(assemble(co * u * v * dx).to_scipy(),
                        bref.matrix(plain * u * v * dx)) < 1e-12, (k, ext)
            _visited(programs, k, ext)
            assert _err(assemble(co * v * dx).get_local(),
                        bref.vector(plain * v * dx)) < 1e-12, (k, ext)
            _visited(programs, k, ext)


def test_newton(hip, case, programs):
    '''tests/test_nonlinear_forms_gpu.py: entries 1e-12 of the largest.  The
    residual c u^2 v dx: k - 1 fields in c, and u.'''
    mesh, spaces, fields = case
    for V in spaces.values():
        v = TestFunction(V)
        u = fem.Function(V)
        xy = V.layout.dof_coords
        u.set_array(1.0 + 0.3 * xy[:, 0] * xy[:, 1])
        for k, ext in _cases(1):
            F = _coefficient(fields, k - 1, ext) * u**2 * v * dx
            plain = _coefficient(fields, k - 1, False) * u**2 * v * dx
            asm = ops.NewtonAssembler(derivative(F, u), F, V, fuse=True)
            A, b = asm.assemble()
            assert asm.fused and asm.jobs[0][0] == 'newton'
            _visited(programs, k, ext)
            assert _err(A.to_scipy(), bref.matrix(derivative(plain, u))) < 1e-12, (k, ext)
            assert _err(b.cpu().numpy(), bref.vector(plain)) < 1e-12, (k, ext)


def test_facet_matrix_and_vector(hip, case, programs):
    '''tests/test_facet_arguments_gpu.py: entries 1e-12 of the largest.'''
    mesh, spaces, fields = case
    for V in spaces.values():
        u, v = TrialFunction(V), TestFunction(V)
        for k, ext in _cases():
            plain = _coefficient(fields, k, False)
            co = _coefficient(fields, k, ext)
            assert _err(assemble(co * u * v * ds).to_scipy(),
                        faref.matrix(plain * u * v * ds)) < 1e-12, (k, ext)
            _visited(programs, k, ext)
            assert _err(assemble(co * v * ds).get_local(),
                        faref.vector(plain * v * ds)) < 1e-12, (k, ext)
            _visited(programs, k, ext)


def test_block_matrix_and_vector(hip, case, programs):
    '''flow_form_block_matrix / _vector launch the element kernels of the
    scalar entry points, block by block.  tests/test_vector_forms_gpu.py:
    entries 1e-12 of the largest.'''
    mesh, spaces, fields = case
    with fem.vector_arguments(True):
        for d in spaces:
            W = fem.VectorFunctionSpace(mesh, 'CG', d)
            u, v = TrialFunction(W), TestFunction(W)
            load = as_vector([1.0, 2.0])
            for k, ext in _cases():
                plain = _coefficient(fields, k, False)
                co = _coefficient(fields, k, ext)
                assert _err(assemble(co * dot(u, v) * dx).to_scipy(),
                            vref.matrix(plain * dot(u, v) * dx)) < 1e-12, (k, ext)
                _visited(programs, k, ext)
                assert _err(assemble(co * dot(load, v) * dx).get_local(),
                            vref.vector(plain * dot(load, v) * dx)) < 1e-12, (k, ext)
                _visited(programs, k, ext)
