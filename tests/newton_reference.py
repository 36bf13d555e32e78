# -*- coding: utf-8 -*-
'''
Host references for derivative() and solve(F == 0): the residuals the
nonlinear tests share, central differences of the host evaluator of
tests/bilinear_reference.py, a numpy interpreter of a Program's instruction
stream next to a direct evaluator of its trees, and Newton's method with the
host evaluator's matrices and scipy's sparse LU.
'''
import numpy

from flow_amd import fem
from flow_amd.fem import (
    forms, TestFunction, dx, dot, inner, grad, sqrt, exp, sin,
    SpatialCoordinate,
    )

import bilinear_reference as bref


def field(V, f):
    u = fem.Function(V)
    xy = V.layout.dof_coords
    u.set_array(f(xy[:, 0], xy[:, 1]))
    return u


def state(V):
    '''A smooth state with 1 <= u <= 2 (abs and u**1.5 are smooth there).'''
    return field(V, lambda x, y: 1.5 + 0.5 * numpy.sin(3.0 * x)
                 * numpy.cos(2.0 * y))


def residuals(mesh, V, u):
    '''[(name, F)] of residuals F(u; v) on V at the Function u.'''
    v = TestFunction(V)
    P2 = fem.FunctionSpace(mesh, 'CG', 2)
    th = field(P2, lambda x, y: 0.5 + numpy.sin(3 * x) * y)
    c = fem.Constant(0.7)
    ex = fem.Expression('exp(x[0]) + x[1]*x[1]', degree=2)
    X = SpatialCoordinate(mesh)
    return [
        ('quasilinear', (1 + u**2) * inner(grad(u), grad(v)) * dx),
        ('minimal surface',
         inner(grad(u), grad(v)) / sqrt(1 + dot(grad(u), grad(u))) * dx),
        ('exp', exp(u) * v * dx),
        ('abs', abs(u) * u * v * dx),
        ('power 1.5', u**1.5 * v * dx),
        ('sin convection', sin(u) * u.dx(0) * v * dx),
        ('field, Constant, Expression',
         ((c * th * u**2 + ex * u) * v
          + (th + X[0]) * u * dot(grad(th), grad(v))) * dx
         - ex * th * v * dx),
        ]


def central_difference(F, u, w, eps):
    '''(F(u + eps w) - F(u - eps w)) / (2 eps) with the host evaluator on the
    unextracted trees; u is restored.'''
    u0 = u.array().copy()
    u.set_array(u0 + eps * w)
    fp = bref.vector(F)
    u.set_array(u0 - eps * w)
    fm = bref.vector(F)
    u.set_array(u0)
    return (fp - fm) / (2.0 * eps)


# -- programs ---------------------------------------------------------------------
class Leaves(object):
    '''Random values (n points) for the leaves of trees, the same for every
    occurrence of a leaf.'''

    def __init__(self, n, seed=0):
        self.n = n
        self.rng = numpy.random.RandomState(seed)
        self.values = {}

    def __call__(self, kind, obj, comp, d=0):
        key = (kind, id(obj), comp, d)
        if key not in self.values:
            if kind == 'num':
                self.values[key] = numpy.full(self.n, float(comp))
            elif kind == 'const':
                self.values[key] = numpy.full(
                    self.n, float(obj.values()[comp]))
            else:
                self.values[key] = self.rng.uniform(0.5, 2.0, self.n)
        return self.values[key]


_UNARY = {'neg': numpy.negative, 'abs': numpy.abs, 'sqrt': numpy.sqrt,
          'exp': numpy.exp, 'ln': numpy.log, 'sin': numpy.sin,
          'cos': numpy.cos}
_BINARY = {'add': numpy.add, 'sub': numpy.subtract, 'mul': numpy.multiply,
           'div': numpy.divide, 'pow': numpy.power}


def eval_tree(n, leaves):
    '''An argument-free scalar tree at the leaf values.'''
    k = n[0]
    if k == 'num':
        return leaves('num', None, n[1])
    if k == 'const':
        return leaves('const', n[1], n[2])
    if k == 'x':
        return leaves('x', None, n[1])
    if k == 'field':
        return leaves('field', n[1], n[2], n[3])
    if k == 'expr':
        return leaves('expr', n[1], n[2])
    a = eval_tree(n[1], leaves)
    if k == 'powi':
        return a**n[2]
    if k in _UNARY:
        return _UNARY[k](a)
    return _BINARY[k](a, eval_tree(n[2], leaves))


def run_program(prog, leaves):
    '''{slot: values} of the instruction stream of a forms.Program: the
    register machine of csrc/form_kernels.hip in numpy.'''
    names = {v: k for k, v in forms.OPS.items()}
    R = [None] * forms.REGISTERS
    out = {}
    for op, dst, a, b in prog.code:
        name = names[op]
        if name == 'out':
            assert b not in out and 0 <= b < prog.nout
            out[b] = R[a].copy()
            continue
        if name == 'const':
            key = prog.consts[a]
            v = leaves('num', None, key[1]) if key[0] == 'num' \
                else leaves('const', key[0], key[1])
        elif name == 'coord':
            v = leaves('x', None, a)
        elif name == 'field':
            v = leaves('field', prog.fields[a][0], prog.fields[a][1], b)
        elif name == 'expr':
            v = leaves('expr', prog.exprs[a][0], prog.exprs[a][1])
        elif name == 'mov':
            v = R[a]
        elif name in _UNARY:
            v = _UNARY[name](R[a])
        else:
            v = _BINARY[name](R[a], R[b])
        assert v is not None, 'read of a register never written'
        assert 0 <= dst < forms.REGISTERS
        R[dst] = numpy.array(v, dtype=float)
    return out


# -- Newton on the host -----------------------------------------------------------
def quasilinear_problem(n, degree):
    '''-div((1 + u^2) grad u) = f on the unit square with u_exact =
    sin(pi x) sin(pi y) and Dirichlet data: (V, u, F, bcs, exact).'''
    mesh = fem.UnitSquareMesh(n, n)
    V = fem.FunctionSpace(mesh, 'CG', degree)
    S = 'sin(pi*x[0])*sin(pi*x[1])'
    g2 = ('pi*pi*(pow(cos(pi*x[0])*sin(pi*x[1]), 2)'
          ' + pow(sin(pi*x[0])*cos(pi*x[1]), 2))')
    exact = fem.Expression(S, degree=5)
    f = fem.Expression('2.0*pi*pi*S*(1.0 + S*S) - 2.0*S*G'
                       .replace('S', '(%s)' % S).replace('G', '(%s)' % g2),
                       degree=5)
    u = fem.Function(V)
    v = TestFunction(V)
    F = (1 + u**2) * inner(grad(u), grad(v)) * dx - f * v * dx
    bcs = [fem.DirichletBC(V, fem.Expression(S, degree=5), 'on_boundary')]
    return V, u, F, bcs, exact


def host_newton(F, u, bcs, J=None, maxit=50, rtol=1.0e-9, atol=1.0e-10,
                relax=1.0):
    '''dolfin's NewtonSolver with the host evaluator's J and F and a sparse
    LU: (residual norms, iterations); the solution is left in u.'''
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla
    V = u.function_space()
    if J is None:
        J = fem.derivative(F, u)
    dofs, g = fem.bcs.collect(list(bcs), V.N)
    keep = numpy.ones(V.N)
    keep[dofs] = 0.0
    K = sp.diags(keep)
    x = u.array().copy()
    x[dofs] = g
    u.set_array(x)
    res = []
    it = 0
    while True:
        A = K.dot(bref.matrix(J)).dot(K) + sp.diags(1.0 - keep)
        b = keep * bref.vector(F)
        res.append(float(numpy.linalg.norm(b)))
        if res[-1] < atol or res[-1] / res[0] < rtol or it == maxit:
            return res, it
        x = x - relax * spla.splu(A.tocsc()).solve(b)
        u.set_array(x)
        it += 1
