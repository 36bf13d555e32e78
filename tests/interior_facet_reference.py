# -*- coding: utf-8 -*-
'''
Host evaluator of interior-facet integrals (`assemble(f*dS)`,
`interior_facet_integrals`, `cell_indicator`; flow_amd/fem/forms.py): numpy,
written from the definition and independent of the device, of the kernel's
rule layout and of the product's facet lists.  It finds the two cells of every
edge by looking the edge's vertex pair up in the cells' vertex triples; '+' is
the cell with the smaller index.  Gauss-Legendre points are placed on the edge
in PHYSICAL coordinates, and each side gets the point's reference coordinates
by inverting its own cell's affine map, so the two sides are matched by where
the point is, not by a permutation of barycentric coordinates.  A side's
normal is the unit edge normal pointing away from that cell's third vertex.
'''
import numpy

from flow_amd.fem import reference


def two_cell_edges(mesh):
    '''(edge ids ascending, (m, 2) their cells with the smaller index first):
    the edges whose vertex pair occurs in exactly two cells.'''
    held = _TWO_CELL_EDGES.get(id(mesh))
    if held is not None and held[0] is mesh:
        return held[1]
    out = _two_cell_edges(mesh)
    _TWO_CELL_EDGES[id(mesh)] = (mesh, out)
    return out


_TWO_CELL_EDGES = {}


def _two_cell_edges(mesh):
    edge_id = dict(((int(a), int(b)), k)
                   for k, (a, b) in enumerate(mesh.edges))
    cells = {}
    for c, tri in enumerate(mesh.cell_vertices):
        for i, j in ((0, 1), (1, 2), (0, 2)):
            a, b = int(tri[i]), int(tri[j])
            cells.setdefault(edge_id[(min(a, b), max(a, b))], []).append(c)
    ids = sorted(k for k, cs in cells.items() if len(cs) == 2)
    assert all(len(cs) in (1, 2) for cs in cells.values())
    return (numpy.array(ids, dtype=numpy.int64),
            numpy.array([sorted(cells[k]) for k in ids], dtype=numpy.int64))


class _Side(object):
    '''One side of the selected facets: the cell, the reference coordinates of
    the facet's points in it, its outward normal, its cell quantities.'''

    def __init__(self, mesh, cells, ev, X):
        self.cells = cells
        a, b = mesh.points[ev[:, 0]], mesh.points[ev[:, 1]]
        cv = mesh.cell_vertices[cells]
        P = mesh.points[cv]                                     # (m, 3, 2)
        off = (cv != ev[:, :1]) & (cv != ev[:, 1:])
        assert (off.sum(axis=1) == 1).all()
        third = P[numpy.arange(len(cells)), off.argmax(axis=1)]
        length = numpy.hypot(*(b - a).T)
        t = (b - a) / length[:, None]
        nrm = numpy.stack([t[:, 1], -t[:, 0]], axis=1)
        nrm[numpy.einsum('md,md->m', nrm, third - a) > 0.0] *= -1.0
        self.normal = nrm
        J = numpy.stack([P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]], axis=2)
        Jinv = numpy.linalg.inv(J)
        self.JinvT = numpy.transpose(Jinv, (0, 2, 1))
        self.ref = numpy.einsum('mrd,mqd->mqr', Jinv, X - P[:, None, 0])
        area = 0.5 * numpy.abs(numpy.linalg.det(J))
        e = numpy.stack([numpy.hypot(*(P[:, 1] - P[:, 0]).T),
                         numpy.hypot(*(P[:, 2] - P[:, 1]).T),
                         numpy.hypot(*(P[:, 0] - P[:, 2]).T)], axis=1)
        self.quantities = [area, e.prod(axis=1) / (4.0 * area), e.max(axis=1)]


class _Facets(object):
    def __init__(self, mesh, q, sel_edges, sel_cells):
        self.mesh = mesh
        ev = mesh.edges[sel_edges].astype(numpy.int64)          # (m, 2)
        a, b = mesh.points[ev[:, 0]], mesh.points[ev[:, 1]]
        x, w = numpy.polynomial.legendre.leggauss(q // 2 + 1)
        s = 0.5 * (x + 1.0)
        self.wts = 0.5 * w
        self.X = a[:, None, :] + s[None, :, None] * (b - a)[:, None, :]
        self.length = numpy.hypot(*(b - a).T)
        self.sides = [_Side(mesh, sel_cells[:, k], ev, self.X)
                      for k in (0, 1)]
        self.arrays = {}

    def shape(self):
        return self.X.shape[:2]

    def field(self, f, comp, d, side):
        S = self.sides[side]
        V = f.function_space()
        if id(f) not in self.arrays:
            self.arrays[id(f)] = f.array().reshape(V.dim, V.N)
        U = self.arrays[id(f)][comp][V.layout.cell_dofs[S.cells]]
        m, nq = self.shape()
        pts = S.ref.reshape(-1, 2)
        if d == 0:
            tab = reference.tabulate(V.degree, pts).reshape(m, nq, -1)
            return numpy.einsum('mj,mqj->mq', U, tab)
        g = reference.tabulate_grad(V.degree, pts).reshape(m, nq, -1, 2)
        gref = numpy.einsum('mj,mqjr->mqr', U, g)
        return numpy.einsum('mr,mqr->mq', S.JinvT[:, d - 1, :], gref)

    def leaf(self, n, side):
        shape = self.shape()
        k = n[0]
        if k == 'field':
            return self.field(n[1], n[2], n[3], side)
        if k == 'n':
            return numpy.repeat(self.sides[side].normal[:, n[1], None],
                                shape[1], axis=1)
        if k == 'cell':
            return numpy.repeat(self.sides[side].quantities[n[2]][:, None],
                                shape[1], axis=1)
        raise ValueError('leaf %r' % (k,))


_UNARY = {'neg': numpy.negative, 'abs': numpy.abs, 'sqrt': numpy.sqrt,
          'exp': numpy.exp, 'ln': numpy.log, 'sin': numpy.sin,
          'cos': numpy.cos, 'sign': numpy.sign, 'tanh': numpy.tanh}
_BINARY = {'add': numpy.add, 'sub': numpy.subtract, 'mul': numpy.multiply,
           'div': numpy.divide, 'pow': numpy.power, 'max': numpy.maximum,
           'min': numpy.minimum}
_COMPARE = {'lt': numpy.less, 'le': numpy.less_equal, 'gt': numpy.greater,
            'ge': numpy.greater_equal, 'eq': numpy.equal,
            'ne': numpy.not_equal}


def _eval(n, F):
    k = n[0]
    shape = F.shape()
    if k == 'num':
        return numpy.full(shape, n[1])
    if k == 'const':
        return numpy.full(shape, float(n[1].values()[n[2]]))
    if k == 'x':
        return F.X[:, :, n[1]]
    if k == 'farea':
        return numpy.repeat(F.length[:, None], shape[1], axis=1)
    if k == 'side':
        return F.leaf(n[1], n[2])
    if k == 'field' and n[3] == 0:
        return F.leaf(n, 0)                 # continuous: evaluated on '+'
    if k == 'cond':
        with numpy.errstate(all='ignore'):
            return numpy.where(_eval(n[1], F) != 0.0, _eval(n[2], F),
                               _eval(n[3], F))
    a = _eval(n[1], F)
    if k == 'powi':
        return a**n[2]
    if k in _UNARY:
        return _UNARY[k](a)
    b = _eval(n[2], F)
    if k in _COMPARE:
        return _COMPARE[k](a, b).astype(float)
    return _BINARY[k](a, b)


def selection(mesh, markers=None, subdomain_id='everywhere'):
    '''(edge ids, their two cells) of the facets a dS integral covers.'''
    ids, cells = two_cell_edges(mesh)
    if subdomain_id in (None, 'everywhere'):
        return ids, cells
    keep = markers.array()[ids] == subdomain_id
    return ids[keep], cells[keep]


def facet_integrals(part):
    '''(edge ids, per-facet integrals) of ONE dS form.'''
    from flow_amd.fem import forms
    assert part.integral_type == 'interior_facet'
    mesh = forms.form_mesh(part.integrand, part.mesh)
    ids, cells = selection(mesh, part.subdomain_data, part.subdomain_id)
    if len(ids) == 0:
        return ids, numpy.zeros(0)
    F = _Facets(mesh, forms.check_degree(part.degree()), ids, cells)
    v = _eval(part.integrand.comps, F)
    return ids, numpy.einsum('mq,q,m->m', v, F.wts, F.length)


def functional(form):
    '''assemble(form) on the host: a dS form, or a signed sum of dx, ds and
    dS forms (tests/form_reference.py, tests/facet_reference.py for those).'''
    import facet_reference
    total = 0.0
    for sign, part in form.terms():
        if part.integral_type == 'interior_facet':
            total += sign * float(facet_integrals(part)[1].sum())
        else:
            total += sign * facet_reference.functional(part)
    return total


def cell_values(part):
    '''(nc,) integrals of ONE dx form over each cell.'''
    import form_reference
    from flow_amd.fem import forms
    mesh = forms.form_mesh(part.integrand, part.mesh)
    cells = form_reference._Cells(mesh, forms.check_degree(part.degree()))
    v = form_reference._eval(part.integrand.comps, cells)
    return numpy.einsum('cq,q,c->c', v, cells.wts, cells.adet)


def cell_shares(form, share=0.5):
    '''cell_indicator(form, share) on the host: every cell gets `share` times
    the integral of each selected interior facet it touches (dS parts) and
    its own integral (dx parts).'''
    from flow_amd.fem import forms
    out = None
    for sign, part in form.terms():
        mesh = forms.form_mesh(part.integrand, part.mesh)
        if out is None:
            out = numpy.zeros(mesh.num_cells())
        if part.integral_type == 'cell':
            out += sign * cell_values(part)
            continue
        ids, vals = facet_integrals(part)
        _, cells = selection(mesh, part.subdomain_data, part.subdomain_id)
        for k in (0, 1):
            numpy.add.at(out, cells[:, k], sign * share * vals)
    return out
