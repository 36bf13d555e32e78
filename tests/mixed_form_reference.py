# -*- coding: utf-8 -*-
'''
Host evaluator of forms of test and trial functions on a Taylor-Hood space
(flow_amd/fem/forms.py, mixed_arguments), numpy / scipy, in the pattern of
tests/vector_form_reference.py and independent of the linearity extraction,
of the 3 x 3 block tables and of the programs: the basis functions phi_i e_r
(r = 0, 1: the velocity basis; r = 2: the pressure basis) are substituted for
the ('arg', number, d, WP, comp) leaves of the UNEXTRACTED integrand tree,
the tree is evaluated at the points of the rule with the bases of BOTH
degrees tabulated there, and the element blocks are scattered through the two
layouts' cell_dofs into a (2 Nv + Np)^2 scipy matrix or a vector of 2 Nv + Np
(velocity x, velocity y, pressure).
'''
import numpy
import scipy.sparse as sp

from flow_amd.fem import forms

import bilinear_reference as bref
import conditional_reference as cref
import facet_reference as facref
import vector_form_reference as vref


class _Cells(vref._Cells):
    def leaf(self, n):
        if n[0] == 'arg':
            if n[4] != self.comp[n[1]]:
                return numpy.zeros(self.shape())
            return self.by_comp[n[4]].cells.arg(n[1], n[2])
        return bref._eval(n, self.cells)


class _Facets(vref._Facets):
    def leaf(self, n):
        if n[0] == 'arg':
            if n[4] != self.comp[n[1]]:
                return numpy.zeros(self.shape())
            other = self.by_comp[n[4]]
            return other.D[n[2]][:, :, other.index[n[1]]]
        return facref._eval(n, self)


def _index(ctx):
    return ctx.cells.index if hasattr(ctx, 'cells') and hasattr(
        ctx.cells, 'index') else ctx.index


def _contexts(part, form_compiler_parameters):
    '''(main context, contexts by component, owning cells, scale).'''
    WP = part.arguments()[0]
    W, P = WP.taylor_hood()
    mesh = WP.mesh()
    q = cref._part_degree(part, form_compiler_parameters)
    made = {}
    for k in (W.degree, P.degree):
        if k in made:
            continue
        if part.integral_type == 'cell':
            scheme = forms.quadrature_scheme(form_compiler_parameters,
                                             part.metadata)
            made[k] = _Cells(mesh, q, scheme, k)
        else:
            sel = facref.selection(mesh, part.subdomain_data,
                                   part.subdomain_id)
            made[k] = _Facets(mesh, q, sel, k)
    by_comp = [made[W.degree], made[W.degree], made[P.degree]]
    main = made[W.degree]
    main.by_comp = by_comp
    if part.integral_type == 'cell':
        cells = numpy.arange(mesh.num_cells())
        if part.subdomain_id not in (None, 'everywhere'):
            cells = numpy.nonzero(
                part.subdomain_data.array() == part.subdomain_id)[0]
        scale = main.cells.wts[None, :] * main.cells.adet[:, None]
        return main, by_comp, cells, scale, True
    return main, by_comp, main.cells, \
        main.wts[None, :] * main.length[:, None], False


def _dofs(WP):
    W, P = WP.taylor_hood()
    return [W.layout.cell_dofs, W.layout.cell_dofs + W.N,
            P.layout.cell_dofs + 2 * W.N]


def _evaluate(tree, main, cells, scale, whole):
    v = cref.evaluate(tree, main) * scale
    if whole:               # (cell contexts hold every cell: dx(k) selects)
        v = v[cells]
    return v.sum(axis=1)


def matrix(form, form_compiler_parameters=None):
    '''assemble(form) of a rank-2 form or sum on a Taylor-Hood space.'''
    total = None
    for sign, part in form.terms():
        WP = part.arguments()[0]
        n = WP.size()
        tree = part.integrand.comps
        dofs = _dofs(WP)
        if part.integral_type != 'cell' and len(facref.selection(
                WP.mesh(), part.subdomain_data, part.subdomain_id)) == 0:
            continue
        main, by_comp, cells, scale, whole = _contexts(
            part, form_compiler_parameters)
        rows, cols, vals = [], [], []
        with numpy.errstate(all='ignore'):
            for r in range(3):
                for s in range(3):
                    main.comp[0], main.comp[1] = r, s
                    for i in range(dofs[r].shape[1]):
                        for j in range(dofs[s].shape[1]):
                            _index(by_comp[r])[0] = i
                            _index(by_comp[s])[1] = j
                            rows.append(dofs[r][cells, i])
                            cols.append(dofs[s][cells, j])
                            vals.append(_evaluate(tree, main, cells, scale,
                                                  whole))
        A = sp.coo_matrix(
            (sign * numpy.concatenate(vals),
             (numpy.concatenate(rows), numpy.concatenate(cols))),
            shape=(n, n)).tocsr()
        total = A if total is None else total + A
    return total


def vector(form, form_compiler_parameters=None):
    '''assemble(form) of a rank-1 form or sum on a Taylor-Hood space.'''
    total = None
    for sign, part in form.terms():
        WP = part.arguments()[0]
        tree = part.integrand.comps
        dofs = _dofs(WP)
        main, by_comp, cells, scale, whole = _contexts(
            part, form_compiler_parameters)
        b = numpy.zeros(WP.size())
        with numpy.errstate(all='ignore'):
            for r in range(3):
                main.comp[0] = r
                for i in range(dofs[r].shape[1]):
                    _index(by_comp[r])[0] = i
                    numpy.add.at(b, dofs[r][cells, i], sign * _evaluate(
                        tree, main, cells, scale, whole))
        total = b if total is None else total + b
    return total
