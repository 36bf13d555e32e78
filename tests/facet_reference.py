# -*- coding: utf-8 -*-
'''
Host evaluator of exterior-facet integrals (`assemble(f*ds)`,
flow_amd/fem/forms.py): numpy, independent of the device and of the kernel's
rule layout.  It walks the boundary edges of the mesh directly: end points
from `mesh.edges`, Gauss-Legendre points on each edge in physical
coordinates, the owning cell found through `bfacet_cell`, the point's
reference coordinates by inverting that cell's affine map, and the outward
normal as the unit edge normal pointing away from the cell's third vertex.
Fields are read with .array(), Expressions through their P_k cell lattice
(as as_cell_coefficient interpolates them).
'''
import numpy

from flow_amd.fem import reference
from flow_amd.fem.function import cell_lattice_points


class _Facets(object):
    def __init__(self, mesh, q, sel):
        self.mesh = mesh
        bf = mesh.bfacets[sel]
        cells = mesh.bfacet_cell[sel]
        self.cells = cells
        ev = mesh.edges[bf]                                     # (m, 2)
        a, b = mesh.points[ev[:, 0]], mesh.points[ev[:, 1]]
        x, w = numpy.polynomial.legendre.leggauss(q // 2 + 1)
        s = 0.5 * (x + 1.0)
        self.wts = 0.5 * w
        self.X = a[:, None, :] + s[None, :, None] * (b - a)[:, None, :]
        self.length = numpy.hypot(*(b - a).T)
        P = mesh.points[mesh.cell_vertices[cells]]              # (m, 3, 2)
        # the cell vertex off the edge
        cv = mesh.cell_vertices[cells]
        off = (cv != ev[:, :1]) & (cv != ev[:, 1:])
        third = P[numpy.arange(len(cells)), off.argmax(axis=1)]
        t = (b - a) / self.length[:, None]
        nrm = numpy.stack([t[:, 1], -t[:, 0]], axis=1)
        flip = numpy.einsum('md,md->m', nrm, third - a) > 0.0
        nrm[flip] *= -1.0
        self.normal = nrm
        J = numpy.stack([P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]], axis=2)
        Jinv = numpy.linalg.inv(J)
        self.JinvT = numpy.transpose(Jinv, (0, 2, 1))
        # reference coordinates of the points in their cells
        self.ref = numpy.einsum('mrd,mqd->mqr', Jinv, self.X - P[:, None, 0])
        self.arrays = {}
        self.lattices = {}

    def shape(self):
        return self.X.shape[:2]

    def field(self, f, comp, d):
        V = f.function_space()
        if id(f) not in self.arrays:
            self.arrays[id(f)] = f.array().reshape(V.dim, V.N)
        U = self.arrays[id(f)][comp][V.layout.cell_dofs[self.cells]]   # (m, nloc)
        m, nq = self.shape()
        pts = self.ref.reshape(-1, 2)
        if d == 0:
            tab = reference.tabulate(V.degree, pts).reshape(m, nq, -1)
            return numpy.einsum('mj,mqj->mq', U, tab)
        g = reference.tabulate_grad(V.degree, pts).reshape(m, nq, -1, 2)
        gref = numpy.einsum('mj,mqjr->mqr', U, g)
        return numpy.einsum('mr,mqr->mq', self.JinvT[:, d - 1, :], gref)

    def expr(self, e, comp):
        k = int(e.degree)
        if id(e) not in self.lattices:
            X = cell_lattice_points(self.mesh, k)
            nc, nl = X.shape[:2]
            self.lattices[id(e)] = e.eval(X.reshape(-1, 2).T).reshape(-1, nc, nl)
        lat = self.lattices[id(e)][comp][self.cells]             # (m, nl)
        m, nq = self.shape()
        tab = reference.tabulate(k, self.ref.reshape(-1, 2)).reshape(m, nq, -1)
        return numpy.einsum('ml,mql->mq', lat, tab)


def _eval(n, F):
    k = n[0]
    shape = F.shape()
    if k == 'num':
        return numpy.full(shape, n[1])
    if k == 'const':
        return numpy.full(shape, float(n[1].values()[n[2]]))
    if k == 'x':
        return F.X[:, :, n[1]]
    if k == 'n':
        return numpy.repeat(F.normal[:, n[1], None], shape[1], axis=1)
    if k == 'field':
        return F.field(n[1], n[2], n[3])
    if k == 'expr':
        return F.expr(n[1], n[2])
    a = _eval(n[1], F)
    if k == 'powi':
        return a**n[2]
    unary = {'neg': numpy.negative, 'abs': numpy.abs, 'sqrt': numpy.sqrt,
             'exp': numpy.exp, 'ln': numpy.log, 'sin': numpy.sin,
             'cos': numpy.cos}
    if k in unary:
        return unary[k](a)
    b = _eval(n[2], F)
    return {'add': numpy.add, 'sub': numpy.subtract, 'mul': numpy.multiply,
            'div': numpy.divide, 'pow': numpy.power}[k](a, b)


def selection(mesh, markers=None, subdomain_id='everywhere'):
    '''Indices into mesh.bfacets of the facets a ds integral covers.'''
    if subdomain_id in (None, 'everywhere'):
        return numpy.arange(len(mesh.bfacets))
    return numpy.nonzero(markers.array()[mesh.bfacets] == subdomain_id)[0]


def functional(form):
    '''assemble(f*ds(...)) on the host, or of a sum of such forms and dx
    forms (tests/form_reference.py for the cells).'''
    from flow_amd.fem import forms
    import form_reference
    total = 0.0
    for sign, part in form.terms():
        if part.integral_type == 'cell':
            total += sign * form_reference.functional(part)
            continue
        mesh = forms.form_mesh(part.integrand, part.mesh)
        sel = selection(mesh, part.subdomain_data, part.subdomain_id)
        F = _Facets(mesh, forms.check_degree(part.degree()), sel)
        v = _eval(part.integrand.comps, F)
        total += sign * float(numpy.einsum('mq,q,m->', v, F.wts, F.length))
    return total
