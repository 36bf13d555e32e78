# -*- coding: utf-8 -*-
'''
Host evaluator of forms of test and trial functions over exterior facets
(`assemble(g*v*ds(k))`, `assemble(h*u*v*ds)`: flow_amd/fem/forms.py), numpy /
scipy, independent of the linearity extraction and of the kernel's rule
layout.  Basis functions i (test) and j (trial) of the owning cell -- ALL of
them, not only those of the edge -- are substituted for the ('arg', ...)
leaves of the UNEXTRACTED integrand, as tests/bilinear_reference.py does over
cells; the tree is evaluated at Gauss-Legendre points placed on the physical
boundary edges with the geometry and the normals of tests/facet_reference.py
(conditional, cell geometry and the other extended nodes through
tests/conditional_reference.py) and scattered through the cell's dofs.
dx parts of a sum go to tests/bilinear_reference.py.
'''
import numpy
import scipy.sparse as sp

from flow_amd.fem import forms, reference

import bilinear_reference as bref
import conditional_reference as cref
import facet_reference as facref


class _Facets(facref._Facets):
    '''The facets of facet_reference with the basis functions of the argument
    space tabulated at the points: D[d][facet, point, i].'''

    def __init__(self, mesh, q, sel, degree):
        facref._Facets.__init__(self, mesh, q, sel)
        m, nq = self.shape()
        pts = self.ref.reshape(-1, 2)
        phi = reference.tabulate(degree, pts).reshape(m, nq, -1)
        g = reference.tabulate_grad(degree, pts).reshape(m, nq, -1, 2)
        self.D = [phi,
                  numpy.einsum('mr,mqir->mqi', self.JinvT[:, 0, :], g),
                  numpy.einsum('mr,mqir->mqi', self.JinvT[:, 1, :], g)]
        self.index = {0: 0, 1: 0}
        self.geometry = cref.cell_quantities(mesh)[self.cells]

    def leaf(self, n):
        if n[0] == 'arg':
            return self.D[n[2]][:, :, self.index[n[1]]]
        return facref._eval(n, self)

    def cell(self, mesh, k):
        return numpy.repeat(self.geometry[:, k, None], self.shape()[1], axis=1)


def element_tensors(part, form_compiler_parameters=None):
    '''(V, owning cells (m,), Ke (m, nloc, nloc)) of a rank-2 ds part, or
    (V, cells, be (m, nloc)) of a rank-1 one; m: the selected facets.'''
    V = part.arguments()[0]
    q = forms._quadrature_degree(part.metadata)
    if q is None:
        q = forms._quadrature_degree(form_compiler_parameters)
    q = forms.check_degree(part.degree() if q is None else q)
    mesh = V.mesh()
    sel = facref.selection(mesh, part.subdomain_data, part.subdomain_id)
    F = _Facets(mesh, q, sel, V.degree)
    nloc = V.layout.nloc
    tree = part.integrand.comps
    rank = len(forms.arguments(tree))
    scale = F.wts[None, :] * F.length[:, None]
    if rank == 1:
        be = numpy.zeros((len(sel), nloc))
        for i in range(nloc):
            F.index[0] = i
            be[:, i] = (cref.evaluate(tree, F) * scale).sum(axis=1)
        return V, F.cells, be
    Ke = numpy.zeros((len(sel), nloc, nloc))
    for i in range(nloc):
        for j in range(nloc):
            F.index[0], F.index[1] = i, j
            Ke[:, i, j] = (cref.evaluate(tree, F) * scale).sum(axis=1)
    return V, F.cells, Ke


def matrix(form, form_compiler_parameters=None):
    '''assemble(form) of a rank-2 form or sum (ds and dx parts) on the host:
    scipy CSR.'''
    total = None
    for sign, part in form.terms():
        if part.integral_type == 'cell':
            A = sign * bref.matrix(part, form_compiler_parameters)
        else:
            V, cells, Ke = element_tensors(part, form_compiler_parameters)
            cd = V.layout.cell_dofs[cells]
            nloc = cd.shape[1]
            rows = numpy.repeat(cd, nloc, axis=1).reshape(-1)
            cols = numpy.tile(cd, (1, nloc)).reshape(-1)
            A = sp.coo_matrix((sign * Ke.reshape(-1), (rows, cols)),
                              shape=(V.N, V.N)).tocsr()
        total = A if total is None else total + A
    return total


def vector(form, form_compiler_parameters=None):
    '''assemble(form) of a rank-1 form or sum (ds and dx parts) on the host.'''
    total = None
    for sign, part in form.terms():
        if part.integral_type == 'cell':
            b = sign * bref.vector(part, form_compiler_parameters)
        else:
            V, cells, be = element_tensors(part, form_compiler_parameters)
            b = numpy.zeros(V.N)
            numpy.add.at(b, V.layout.cell_dofs[cells], sign * be)
        total = b if total is None else total + b
    return total


def touched_dofs(V, markers=None, subdomain_id='everywhere'):
    '''Boolean mask of the dofs of the cells that own a selected facet.'''
    mesh = V.mesh()
    sel = facref.selection(mesh, markers, subdomain_id)
    mask = numpy.zeros(V.N, dtype=bool)
    mask[V.layout.cell_dofs[mesh.bfacet_cell[sel]].reshape(-1)] = True
    return mask


def host_newton(F, u, bcs, J, maxit=50, rtol=1.0e-9, atol=1.0e-10):
    '''dolfin's NewtonSolver with this evaluator's J and F and a sparse LU, as
    newton_reference.host_newton does for dx forms: (residual norms,
    iterations); the solution is left in u.'''
    import scipy.sparse.linalg as spla
    from flow_amd import fem
    V = u.function_space()
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
        A = K.dot(matrix(J)).dot(K) + sp.diags(1.0 - keep)
        b = keep * vector(F)
        res.append(float(numpy.linalg.norm(b)))
        if res[-1] < atol or res[-1] / res[0] < rtol or it == maxit:
            return res, it
        x = x - spla.splu(A.tocsc()).solve(b)
        u.set_array(x)
        it += 1
