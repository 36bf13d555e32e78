# -*- coding: utf-8 -*-
'''
Host evaluator of the integrands of flow_amd/fem/forms.py: numpy, the same
scalar trees at the same quadrature rules (reference.triangle_rule) as the
form kernels, independent of the register programs and of the device.
Functions are read with .array(); Expressions through their P_k cell lattice,
as as_cell_coefficient interpolates them.
'''
import numpy

from flow_amd.fem import reference
from flow_amd.fem.function import cell_lattice_points


class _Cells(object):
    def __init__(self, mesh, q):
        self.mesh = mesh
        self.pts, self.wts = reference.triangle_rule(q)
        P = mesh.points[mesh.cell_vertices]                     # (Nc, 3, 2)
        lat = numpy.stack([1.0 - self.pts[:, 0] - self.pts[:, 1],
                           self.pts[:, 0], self.pts[:, 1]], axis=1)   # (nq, 3)
        self.X = numpy.einsum('qv,cvd->cqd', lat, P)             # (Nc, nq, 2)
        J = numpy.stack([P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]], axis=2)
        self.adet = numpy.abs(numpy.linalg.det(J))
        self.JinvT = numpy.transpose(numpy.linalg.inv(J), (0, 2, 1))
        self.arrays = {}
        self.lattices = {}

    def field(self, f, comp, d):
        V = f.function_space()
        if id(f) not in self.arrays:
            self.arrays[id(f)] = f.array().reshape(V.dim, V.N)
        U = self.arrays[id(f)][comp][V.layout.cell_dofs]         # (Nc, nloc)
        if d == 0:
            return U.dot(reference.tabulate(V.degree, self.pts).T)
        g = reference.tabulate_grad(V.degree, self.pts)          # (nq, nloc, 2)
        gref = numpy.einsum('cj,qjr->cqr', U, g)
        return numpy.einsum('cr,cqr->cq', self.JinvT[:, d - 1, :], gref)

    def expr(self, e, comp):
        k = int(e.degree)
        if id(e) not in self.lattices:
            X = cell_lattice_points(self.mesh, k)
            nc, nl = X.shape[:2]
            self.lattices[id(e)] = e.eval(X.reshape(-1, 2).T).reshape(-1, nc, nl)
        return self.lattices[id(e)][comp].dot(reference.tabulate(k, self.pts).T)


def _eval(n, cells):
    k = n[0]
    if k == 'num':
        return numpy.full(cells.X.shape[:2], n[1])
    if k == 'const':
        return numpy.full(cells.X.shape[:2], float(n[1].values()[n[2]]))
    if k == 'x':
        return cells.X[:, :, n[1]]
    if k == 'field':
        return cells.field(n[1], n[2], n[3])
    if k == 'expr':
        return cells.expr(n[1], n[2])
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


def functional(form, mesh=None):
    '''assemble(form) on the host.'''
    from flow_amd.fem import forms
    mesh = forms.form_mesh(form.integrand, form.mesh if mesh is None else mesh)
    cells = _Cells(mesh, forms.check_degree(form.degree()))
    v = _eval(form.integrand.comps, cells)
    return float(numpy.einsum('cq,q,c->', v, cells.wts, cells.adet))


def load_vector(expr, V, form_compiler_parameters=None):
    '''b_(a,i) = int expr_a phi_i on the host (component-blocked).'''
    from flow_amd.fem import forms
    mesh = V.mesh()
    q = forms.projection_degree(expr, V.degree, form_compiler_parameters)
    cells = _Cells(mesh, q)
    phi = reference.tabulate(V.degree, cells.pts)               # (nq, nloc)
    cd = V.layout.cell_dofs                                     # (Nc, nloc)
    out = numpy.zeros((V.dim, V.N))
    for a, t in enumerate(expr.scalar_trees()):
        v = _eval(t, cells)
        loc = numpy.einsum('cq,q,c,qi->ci', v, cells.wts, cells.adet, phi)
        numpy.add.at(out[a], cd, loc)
    return out.reshape(-1)
