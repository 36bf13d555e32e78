# -*- coding: utf-8 -*-
'''
The cases of form assembly that tests/test_form_jobs_host.py (job lists, on
the host) and tools/form_assembly_gate.py (results and launch counts against
another tree, on the GPU) share: (J, F) pairs on scalar and vector spaces and
one-shot forms of ranks 1 and 2.  The callers switch vector_arguments,
vector_derivatives and facet_arguments on (switches()).
'''
from flow_amd import fem
from flow_amd.fem import (
    TestFunction, TrialFunction, dx, Measure, MeshFunction, dot, inner, grad,
    derivative, SpatialCoordinate, as_vector, sin, cos,
    )

import newton_reference as nref
import vector_newton_reference as vnref

VERTEX = {'quadrature_rule': 'vertex'}


def square_markers(mesh):
    '''1 left, 2 right, 3 top; the bottom stays 0.'''
    m = MeshFunction('size_t', mesh, 1, 0)
    vnref.Side(lambda x: x[0] < 1e-12).mark(m, 1)
    vnref.Side(lambda x: x[0] > 1.0 - 1e-12).mark(m, 2)
    vnref.Side(lambda x: x[1] > 1.0 - 1e-12).mark(m, 3)
    return m


def remark(markers):
    '''Other facets behind the same ids: 1 bottom, 2 left, 3 right.'''
    markers.set_all(0)
    vnref.Side(lambda x: x[1] < 1e-12).mark(markers, 1)
    vnref.Side(lambda x: x[0] < 1e-12).mark(markers, 2)
    vnref.Side(lambda x: x[0] > 1.0 - 1e-12).mark(markers, 3)


class Case(object):
    '''One (J, F) pair: name, space, state u, a Constant of the forms, the
    facet markers (or None), the arguments of newton_jobs.'''

    def __init__(self, name, V, u, J, F, const, markers=None, fuse=True):
        self.name = 'P%d %s' % (V.degree, name)
        self.V, self.u, self.J, self.F = V, u, J, F
        self.const, self.markers, self.fuse = const, markers, fuse


def scalar_cases(mesh, V):
    v = TestFunction(V)
    u = nref.state(V)
    c = fem.Constant(0.7)
    f = fem.Expression('1.0 + x[0]*x[1]', degree=2)
    markers = square_markers(mesh)
    dsm = Measure('ds', domain=mesh, subdomain_data=markers)
    q = (1 + u**2) * inner(grad(u), grad(v)) * dx
    F = q - c * f * v * dx
    J = derivative(F, u)
    yield Case('fused pair', V, u, J, F, c)
    yield Case('fuse=False', V, u, J, F, c, fuse=False)
    G = (1 + c * u**2) * inner(grad(u), grad(v)) * dx(degree=3)
    yield Case('other degree', V, u, J, G, c)
    M = dict(nref.residuals(mesh, V, u))['minimal surface'] + c * u * v * dx
    yield Case('two programs', V, u, derivative(M, u), M, c)
    R = q + c * u**2 * v * dsm(1) - f * v * dsm(2) + u * v * dx
    yield Case('ds in J and F', V, u, derivative(R, u), R, c, markers)
    N = -(c * u**3 * v * dx) + inner(grad(u), grad(v)) * dx
    yield Case('first sign -1', V, u, derivative(N, u), N, c)


def vector_cases(mesh, W):
    for name, u, F, _ in vnref.residuals(W):
        markers = None
        const = fem.Constant(1.0)
        v = TestFunction(W)
        if name == 'traction robin':
            markers = vnref.x_markers(mesh)
            F = vnref.traction_robin(W, u, markers)[0]
        F = F + const * dot(u, v) * dx(degree=1)
        yield Case(name, W, u, derivative(F, u), F, const, markers)
    u = vnref.state(W)
    v = TestFunction(W)
    nu = fem.Constant(0.05)
    f = fem.Expression(vnref.SOURCE, degree=2)
    F = (nu * inner(grad(u), grad(v)) + dot(dot(grad(u), u), v)) * dx \
        - dot(f, v) * dx
    J = derivative(F, u)
    yield Case('burgers, source apart', W, u, J, F, nu)
    yield Case('burgers, fuse=False', W, u, J, F, nu, fuse=False)


def _long(X, k):
    """A coefficient of about twenty instructions, different for every k."""
    return (sin((1.0 + 0.25 * k) * X[0]) * cos(X[1] - 0.5 * k)
            + (0.5 + k) * X[0] * X[1] + 1.0 / (2.0 + k + X[1] * X[1]))


def long_integrands(mesh, W):
    """(rank-2, rank-1) integrands whose block (0, 0) / 0 has nine / three
    long coefficients, more than one program holds, next to blocks of one
    program (test_vector_forms_gpu.test_blocks_of_several_programs uses
    them too)."""
    X = SpatialCoordinate(mesh)
    u, v = TrialFunction(W), TestFunction(W)
    c = [_long(X, k) for k in range(9)]
    K = as_vector([[3.0 + c[0], c[1]], [c[2], 3.0 + c[3]]])
    a = (dot(dot(K, grad(u[0])), grad(v[0]))
         + dot(as_vector([c[4], c[5]]), grad(u[0])) * v[0]
         + u[0] * dot(as_vector([c[6], c[7]]), grad(v[0]))
         + c[8] * u[0] * v[0] + c[1] * u[1] * v[1] + c[2] * u[0].dx(1) * v[1])
    L = (c[0] * c[6] * v[0]
         + dot(as_vector([c[1] * c[2], c[3] * c[4]]), grad(v[0]))
         + c[5] * v[1])
    return a, L


def one_shot_forms(mesh):
    '''[(name, form, form_compiler_parameters)] of ranks 1 and 2.'''
    out = []
    markers = square_markers(mesh)
    dsm = Measure('ds', domain=mesh, subdomain_data=markers)
    for k in (1, 2):
        V = fem.FunctionSpace(mesh, 'CG', k)
        u, v = TrialFunction(V), TestFunction(V)
        w = nref.state(V)
        a0, a1, a2 = inner(grad(u), grad(v)) * dx, w * u * v * dx, \
            w**2 * u.dx(0) * v * dx
        L0, L1, L2 = w * v * dx, w**2 * v.dx(1) * dx, v * dx
        tag = 'P%d ' % k
        out += [
            (tag + 'stiffness', a0, None), (tag + 'load', L0, None),
            (tag + '+-+ matrix', a0 - a1 + a2, None),
            (tag + '+-+ vector', L0 - L1 + L2, None),
            (tag + 'ds first matrix', w * u * v * dsm(1) + a0, None),
            (tag + 'ds first vector', w * v * dsm(2) - L1, None),
            (tag + 'ds(99) matrix', a0 + u * v * dsm(99), None),
            (tag + 'ds(99) vector', w * v * dsm(99), None),
            (tag + 'ds(99) first', u * v * dsm(99) + a1, None),
            (tag + 'vertex matrix', a1, VERTEX), (tag + 'vertex vector', L0, VERTEX),
            (tag + 'degree= matrix', w * u * v * dx(degree=1) + a0, None),
            (tag + 'degree= vector', w * v * dx(degree=4) - L2, None),
            ]
        W = fem.VectorFunctionSpace(mesh, 'CG', k)
        U, Vt = TrialFunction(W), TestFunction(W)
        s = vnref.state(W)
        b0 = inner(grad(U), grad(Vt)) * dx
        b1 = U[0].dx(1) * Vt[1] * dx                    # (blocks absent)
        b2 = dot(s, s) * dot(U, Vt) * dsm(1)
        l0 = dot(s, Vt) * dx
        l1 = s[0] * Vt[1] * dx                          # (a component absent)
        l2 = dot(s, Vt) * dsm(3)
        ia, iL = long_integrands(mesh, W)
        tag = 'P%d vector ' % k
        out += [
            (tag + 'laplacian', b0, None), (tag + 'absent block', b1, None),
            (tag + 'absent first', b1 + b0, None),
            (tag + '+-+ matrix', b0 - b1 + b2, None),
            (tag + 'ds first matrix', b2 + b0, None),
            (tag + 'ds(99) matrix', dot(U, Vt) * dsm(99) + b1, None),
            (tag + 'load', l0, None), (tag + 'absent component', l1, None),
            (tag + '+-+ vector', l0 - l1 + l2, None),
            (tag + 'ds first vector', l2 - l0, None),
            (tag + 'ds(99) vector', dot(s, Vt) * dsm(99), None),
            (tag + 'vertex matrix', dot(s, s) * dot(U, Vt) * dx, VERTEX),
            (tag + 'vertex vector', l0, VERTEX),
            (tag + 'degree= matrix', dot(U, Vt) * dx(degree=1) - b0, None),
            (tag + 'several dx matrix', ia * dx, None),
            (tag + 'several dx vector', iL * dx, None),
            (tag + 'several ds matrix', ia * dsm(2), None),
            (tag + 'several ds vector', iL * dsm(2), None),
            (tag + 'several dx + ds', ia * dx + ia * dsm(3), None),
            ]
    return out


def switches():
    fem.vector_arguments(True)
    fem.vector_derivatives(True)
    fem.facet_arguments(True)


def all_cases(mesh):
    out = []
    for k in (1, 2):
        out += list(scalar_cases(mesh, fem.FunctionSpace(mesh, 'CG', k)))
    for k in (1, 2):
        out += list(vector_cases(mesh, fem.VectorFunctionSpace(mesh, 'CG', k)))
    return out
