# -*- coding: utf-8 -*-
'''
Host evaluator of forms of test and trial functions on a VECTOR space
(flow_amd/fem/forms.py, vector_arguments), numpy / scipy, independent of the
linearity extraction, of the block tables and of the programs: the vector
basis functions phi_i e_r (test) and phi_j e_s (trial) are substituted for
the ('arg', number, d, W, comp) leaves of the UNEXTRACTED integrand tree -- a
leaf of component comp is D_d phi where comp is the component of the basis
function and zero elsewhere --, the tree is evaluated at the points of the
rule (cells: tests/bilinear_reference.py; exterior facets:
tests/facet_argument_reference.py; the extended nodes through
tests/conditional_reference.py) and scattered into a 2N x 2N scipy matrix or
a vector of 2N in operator numbering (r*N + i).
'''
import numpy
import scipy.sparse as sp

from flow_amd.fem import forms

import bilinear_reference as bref
import conditional_reference as cref
import facet_argument_reference as faref
import facet_reference as facref


class _Cells(cref.CellContext):
    def __init__(self, mesh, q, scheme, degree):
        cref.CellContext.__init__(self, mesh, q, scheme, degree)
        self.comp = {0: 0, 1: 0}

    def leaf(self, n):
        if n[0] == 'arg':
            if n[4] != self.comp[n[1]]:
                return numpy.zeros(self.shape())
            return self.cells.arg(n[1], n[2])
        return bref._eval(n, self.cells)


class _Facets(faref._Facets):
    def __init__(self, mesh, q, sel, degree):
        faref._Facets.__init__(self, mesh, q, sel, degree)
        self.comp = {0: 0, 1: 0}

    def leaf(self, n):
        if n[0] == 'arg':
            if n[4] != self.comp[n[1]]:
                return numpy.zeros(self.shape())
            return self.D[n[2]][:, :, self.index[n[1]]]
        return facref._eval(n, self)


def _context(part, form_compiler_parameters):
    '''(W, context, index dict, owning cells, scale) of a part.'''
    W = part.arguments()[0]
    q = cref._part_degree(part, form_compiler_parameters)
    mesh = W.mesh()
    if part.integral_type == 'cell':
        scheme = forms.quadrature_scheme(form_compiler_parameters,
                                         part.metadata)
        ctx = _Cells(mesh, q, scheme, W.degree)
        cells = numpy.arange(mesh.num_cells())
        return W, ctx, ctx.cells.index, cells, \
            ctx.cells.wts[None, :] * ctx.cells.adet[:, None]
    sel = facref.selection(mesh, part.subdomain_data, part.subdomain_id)
    ctx = _Facets(mesh, q, sel, W.degree)
    return W, ctx, ctx.index, ctx.cells, ctx.wts[None, :] * ctx.length[:, None]


def element_tensors(part, form_compiler_parameters=None):
    '''(W, owning cells (m,), Ke (m, 2, nloc, 2, nloc)) of a rank-2 part
    (Ke[c, r, i, s, j]) or (W, cells, be (m, 2, nloc)) of a rank-1 part.'''
    tree = part.integrand.comps
    rank = len(forms.arguments(tree))
    W = part.arguments()[0]
    nloc = W.layout.nloc
    if part.integral_type != 'cell' and len(facref.selection(
            W.mesh(), part.subdomain_data, part.subdomain_id)) == 0:
        # an empty selection, ds(99): no facet, no contribution
        return W, numpy.zeros(0, dtype=int), numpy.zeros(
            (0, 2, nloc, 2, nloc) if rank == 2 else (0, 2, nloc))
    W, ctx, index, cells, scale = _context(part, form_compiler_parameters)
    m = len(cells)
    with numpy.errstate(all='ignore'):
        if rank == 1:
            be = numpy.zeros((m, 2, nloc))
            for r in range(2):
                for i in range(nloc):
                    ctx.comp[0], index[0] = r, i
                    be[:, r, i] = (cref.evaluate(tree, ctx) * scale).sum(axis=1)
            return W, cells, be
        Ke = numpy.zeros((m, 2, nloc, 2, nloc))
        for r in range(2):
            for s in range(2):
                for i in range(nloc):
                    for j in range(nloc):
                        ctx.comp[0], ctx.comp[1] = r, s
                        index[0], index[1] = i, j
                        Ke[:, r, i, s, j] = (cref.evaluate(tree, ctx)
                                             * scale).sum(axis=1)
    return W, cells, Ke


def matrix(form, form_compiler_parameters=None):
    '''assemble(form) of a rank-2 form or sum on a vector space: 2N x 2N
    scipy CSR.'''
    total = None
    for sign, part in form.terms():
        W, cells, Ke = element_tensors(part, form_compiler_parameters)
        N = W.N
        cd = W.layout.cell_dofs[cells]                          # (m, nloc)
        dofs = numpy.stack([cd, cd + N], axis=1).reshape(
            len(cells), 2 * cd.shape[1])
        n2 = dofs.shape[1]
        rows = numpy.repeat(dofs, n2, axis=1).reshape(-1)
        cols = numpy.tile(dofs, (1, n2)).reshape(-1)
        A = sp.coo_matrix((sign * Ke.reshape(-1), (rows, cols)),
                          shape=(2 * N, 2 * N)).tocsr()
        total = A if total is None else total + A
    return total


def vector(form, form_compiler_parameters=None):
    '''assemble(form) of a rank-1 form or sum on a vector space: 2N.'''
    total = None
    for sign, part in form.terms():
        W, cells, be = element_tensors(part, form_compiler_parameters)
        N = W.N
        cd = W.layout.cell_dofs[cells]
        dofs = numpy.stack([cd, cd + N], axis=1)                # (m, 2, nloc)
        b = numpy.zeros(2 * N)
        numpy.add.at(b, dofs, sign * be)
        total = b if total is None else total + b
    return total
