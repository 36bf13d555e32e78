# -*- coding: utf-8 -*-
'''
Host evaluator of forms of test and trial functions (flow_amd/fem/forms.py),
independent of the linearity extraction: basis functions i (test) and j (trial)
are substituted for the ('arg', ...) leaves of the UNEXTRACTED integrand tree,
the tree is evaluated with numpy at the points of reference.triangle_rule(q)
(or of the vertex rule) and summed into a scipy.sparse matrix or a vector.
It checks the extraction, the program compiler and the kernels together.
'''
import numpy
import scipy.sparse as sp

from flow_amd.fem import reference, forms

import form_reference as fref


class _Cells(fref._Cells):
    '''The cells of form_reference with the rule left to the caller and the
    basis functions of the argument space tabulated at its points.'''

    def __init__(self, mesh, q, scheme, degree):
        fref._Cells.__init__(self, mesh, q)
        if scheme == 'vertex':
            self.pts = numpy.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]])
            self.wts = numpy.full(3, 1.0 / 6.0)
            P = mesh.points[mesh.cell_vertices]
            lat = numpy.stack([1.0 - self.pts[:, 0] - self.pts[:, 1],
                               self.pts[:, 0], self.pts[:, 1]], axis=1)
            self.X = numpy.einsum('qv,cvd->cqd', lat, P)
        nc = mesh.num_cells()
        phi = reference.tabulate(degree, self.pts)              # (nq, nloc)
        g = reference.tabulate_grad(degree, self.pts)           # (nq, nloc, 2)
        # D[d][c, q, i]: value, d/dx, d/dy of basis function i
        self.D = [numpy.broadcast_to(phi, (nc,) + phi.shape),
                  numpy.einsum('cr,qir->cqi', self.JinvT[:, 0, :], g),
                  numpy.einsum('cr,qir->cqi', self.JinvT[:, 1, :], g)]
        self.index = {0: 0, 1: 0}

    def arg(self, number, d):
        return self.D[d][:, :, self.index[number]]


def _eval(n, cells):
    k = n[0]
    if k == 'arg':
        return cells.arg(n[1], n[2])
    if k in ('num', 'const', 'x', 'field', 'expr'):
        return fref._eval(n, cells)
    a = _eval(n[1], cells)
    if k == 'powi':
        return a**n[2]
    unary = {'neg': numpy.negative, 'abs': numpy.abs, 'sqrt': numpy.sqrt,
             'exp': numpy.exp, 'ln': numpy.log, 'sin': numpy.sin,
             'cos': numpy.cos}
    if k in unary:
        return unary[k](a)
    b = _eval(n[2], cells)
    return {'add': numpy.add, 'sub': numpy.subtract, 'mul': numpy.multiply,
            'div': numpy.divide, 'pow': numpy.power}[k](a, b)


def _setup(part, form_compiler_parameters):
    V = part.arguments()[0]
    q = forms._quadrature_degree(part.metadata)
    if q is None:
        q = forms._quadrature_degree(form_compiler_parameters)
    q = forms.check_degree(part.degree() if q is None else q)
    scheme = forms.quadrature_scheme(form_compiler_parameters, part.metadata)
    return V, _Cells(V.mesh(), q, scheme, V.degree)


def element_tensors(part, form_compiler_parameters=None):
    '''(V, Ke (Nc, nloc, nloc)) of a rank-2 form, or (V, be (Nc, nloc)) of a
    rank-1 form.'''
    V, cells = _setup(part, form_compiler_parameters)
    nloc = V.layout.nloc
    nc = V.mesh().num_cells()
    tree = part.integrand.comps
    rank = len(forms.arguments(tree))
    scale = cells.wts[None, :] * cells.adet[:, None]
    if rank == 1:
        be = numpy.zeros((nc, nloc))
        for i in range(nloc):
            cells.index[0] = i
            be[:, i] = (_eval(tree, cells) * scale).sum(axis=1)
        return V, be
    Ke = numpy.zeros((nc, nloc, nloc))
    for i in range(nloc):
        for j in range(nloc):
            cells.index[0], cells.index[1] = i, j
            Ke[:, i, j] = (_eval(tree, cells) * scale).sum(axis=1)
    return V, Ke


def matrix(form, form_compiler_parameters=None):
    '''assemble(form) of a rank-2 form or sum on the host: scipy CSR.'''
    total = None
    for sign, part in form.terms():
        V, Ke = element_tensors(part, form_compiler_parameters)
        cd = V.layout.cell_dofs                                 # (Nc, nloc)
        nloc = cd.shape[1]
        rows = numpy.repeat(cd, nloc, axis=1).reshape(-1)
        cols = numpy.tile(cd, (1, nloc)).reshape(-1)
        A = sp.coo_matrix((sign * Ke.reshape(-1), (rows, cols)),
                          shape=(V.N, V.N)).tocsr()
        total = A if total is None else total + A
    return total


def vector(form, form_compiler_parameters=None):
    '''assemble(form) of a rank-1 form or sum on the host.'''
    total = None
    for sign, part in form.terms():
        V, be = element_tensors(part, form_compiler_parameters)
        b = numpy.zeros(V.N)
        numpy.add.at(b, V.layout.cell_dofs, sign * be)
        total = b if total is None else total + b
    return total
