# -*- coding: utf-8 -*-
'''
Host references for the extended vocabulary of flow_amd/fem/forms.py:
conditional and its conditions, max_value / min_value / sign / tanh, the cell
geometry operands and the SUPG tau operand.  `evaluate` handles those node
kinds itself (numpy.where for the select: the untaken value never reaches the
result) and hands the leaves to the evaluators of tests/form_reference.py,
tests/bilinear_reference.py, tests/facet_reference.py and
tests/point_reference.py, the old operators to the numpy tables of
tests/newton_reference.py.  On top of it: functionals over cells and facets,
vectors, matrices, values at points, central differences, the numpy
interpreter of an instruction stream with the new opcodes, and the host
Newton iteration.
'''
import numpy
import scipy.sparse as sp

from flow_amd import fem
from flow_amd.fem import forms, reference

import bilinear_reference as bref
import facet_reference as facref
import newton_reference as nref
import point_reference as pref

_COMPARE = {'lt': numpy.less, 'le': numpy.less_equal, 'gt': numpy.greater,
            'ge': numpy.greater_equal, 'eq': numpy.equal,
            'ne': numpy.not_equal}
_UNARY = dict(nref._UNARY, sign=numpy.sign, tanh=numpy.tanh)
_BINARY = dict(nref._BINARY, max=numpy.maximum, min=numpy.minimum)


def evaluate(n, ctx):
    '''The scalar tree n in the context ctx: ctx.leaf(n) evaluates a leaf,
    ctx.cell(mesh, k) a geometry operand, ctx.lattice(obj) an operand with a
    lattice of its own (SUPG tau).'''
    k = n[0]
    if k == 'cell':
        return ctx.cell(n[1], n[2])
    if k == 'expr' and hasattr(n[1], 'form_lattice'):
        return ctx.lattice(n[1])
    if k not in forms.NONLEAF:
        return ctx.leaf(n)
    if k == 'cond':
        c, t, f = [evaluate(m, ctx) for m in n[1:]]
        return numpy.where(c != 0.0, t, f)
    a = evaluate(n[1], ctx)
    if k == 'powi':
        return a**n[2]
    if k in _UNARY:
        return _UNARY[k](a)
    b = evaluate(n[2], ctx)
    if k in _COMPARE:
        return _COMPARE[k](a, b).astype(float)
    return _BINARY[k](a, b)


# -- geometry and tau on the host -------------------------------------------------
def cell_quantities(mesh):
    '''(Nc, 3): |T|, circumradius abc / (4 |T|), largest vertex distance.'''
    P = mesh.points[mesh.cell_vertices]                          # (Nc, 3, 2)
    e = numpy.stack([numpy.hypot(*(P[:, i] - P[:, j]).T)
                     for i, j in ((1, 0), (2, 1), (0, 2))], axis=1)
    J = numpy.stack([P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]], axis=2)
    area = 0.5 * numpy.abs(numpy.linalg.det(J))
    return numpy.stack([area, e.prod(axis=1) / (4.0 * area), e.max(axis=1)],
                       axis=1)


# {id(tau): (Nc, 3) vertex values}: where a test hands the evaluator the
# lattice of a tau (lattice_values), the evaluator interpolates THOSE values.
# The formula of tau cancels for small Pe (one rounding of tanh moves tau by
# 2.2e-16 eps p / |b|^2), so two fp64 evaluations of it agree only as far as
# its conditioning allows; a test of the interpolation and assembly of tau
# takes the values as data, as it takes a Function's, and the values are
# checked on their own.
GIVEN_LATTICES = {}


def lattice_values(tau):
    held = GIVEN_LATTICES.get(id(tau))
    return supg_tau(tau) if held is None else held[1]


def give_lattice(tau, values):
    GIVEN_LATTICES[id(tau)] = (tau, numpy.asarray(values, dtype=float))


def supg_tau(tau):
    '''(Nc, 3): the SUPG parameter of the reference's SupgStab::eval at the
    three vertices of every cell, the convection there being its vertex dof
    value.'''
    mesh, eps, p = tau.mesh, tau.epsilon, tau.p
    W = tau.convection.function_space()
    B = tau.convection.array().reshape(2, W.N)[:, W.layout.cell_dofs[:, :3]]
    bx, by = B[0], B[1]                                           # (Nc, 3)
    P = mesh.points[mesh.cell_vertices]
    area = cell_quantities(mesh)[:, 0]
    nb = numpy.sqrt(bx * bx + by * by)
    total = numpy.zeros_like(nb)
    for i in range(3):
        for j in range(i + 1, 3):
            e0 = (P[:, i, 0] - P[:, j, 0])[:, None]
            e1 = (P[:, i, 1] - P[:, j, 1])[:, None]
            total += numpy.abs(e1 * bx - e0 * by)
    with numpy.errstate(all='ignore'):
        h = 4.0 * nb * area[:, None] / total
        Pe = 0.5 * nb * h / (p * eps)
        xi = numpy.where(Pe > 1.0e-5, (1.0 / numpy.tanh(Pe) - 1.0 / Pe) / Pe,
                         1.0 / 3.0 - Pe * Pe / 45.0 + 2.0 / 945.0 * Pe**4)
        out = h * h / 4.0 / eps / p * xi
    return numpy.where(nb < 1.0e-10, 0.0, out)


# -- contexts -----------------------------------------------------------------------
class CellContext(object):
    '''The points of a rule on every cell: bilinear_reference's _Cells
    (leaves, fields, Expressions and the basis functions standing for the
    arguments).'''

    def __init__(self, mesh, q, scheme='default', degree=1):
        self.mesh = mesh
        self.cells = bref._Cells(mesh, q, scheme, degree)

    def shape(self):
        return self.cells.X.shape[:2]

    def leaf(self, n):
        return bref._eval(n, self.cells)

    def cell(self, mesh, k):
        assert mesh is self.mesh
        return numpy.repeat(cell_quantities(mesh)[:, k, None], self.shape()[1],
                            axis=1)

    def lattice(self, obj):
        return lattice_values(obj).dot(reference.tabulate(1, self.cells.pts).T)


class FacetContext(object):
    def __init__(self, mesh, q, sel):
        self.mesh = mesh
        self.F = facref._Facets(mesh, q, sel)

    def leaf(self, n):
        return facref._eval(n, self.F)

    def cell(self, mesh, k):
        assert mesh is self.mesh
        return numpy.repeat(cell_quantities(mesh)[self.F.cells, k, None],
                            self.F.shape()[1], axis=1)

    def lattice(self, obj):
        m, nq = self.F.shape()
        tab = reference.tabulate(1, self.F.ref.reshape(-1, 2)).reshape(m, nq, 3)
        return numpy.einsum('ml,mql->mq', lattice_values(obj)[self.F.cells],
                            tab)


class PointContext(object):
    '''Located points (pts (n, 2) on the cells (n,)): values of fields,
    coordinates, constants and cell geometry.'''

    def __init__(self, mesh, pts, cells):
        self.mesh, self.pts, self.cells = mesh, pts, cells

    def leaf(self, n):
        k = n[0]
        if k == 'num':
            return numpy.full(len(self.pts), n[1])
        if k == 'const':
            return numpy.full(len(self.pts), float(n[1].values()[n[2]]))
        if k == 'x':
            return self.pts[:, n[1]]
        assert k == 'field', n
        if n[3] == 0:
            return pref.field_values(n[1], self.pts, self.cells)[n[2]]
        # d/dx, d/dy: reference gradients through the cell's Jacobian
        V = n[1].function_space()
        lam = pref.barycentric_own(self.mesh, self.pts, self.cells)
        g = reference.tabulate_grad(V.degree, lam[1:].T)        # (n, nloc, 2)
        U = n[1].array().reshape(V.dim, V.N)[n[2]][
            V.layout.cell_dofs[self.cells]]                      # (n, nloc)
        P = self.mesh.points[self.mesh.cell_vertices[self.cells]]
        J = numpy.stack([P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]], axis=2)
        JinvT = numpy.transpose(numpy.linalg.inv(J), (0, 2, 1))
        gref = numpy.einsum('nj,njr->nr', U, g)
        return numpy.einsum('nr,nr->n', JinvT[:, n[3] - 1, :], gref)

    def cell(self, mesh, k):
        assert mesh is self.mesh
        return cell_quantities(mesh)[self.cells, k]


class LeafContext(object):
    '''Random leaf values (newton_reference.Leaves), the same for every
    occurrence of a leaf: what run_program and eval_tree share.'''

    def __init__(self, leaves):
        self.leaves = leaves

    def leaf(self, n):
        return nref.eval_tree(n, self.leaves)

    def cell(self, mesh, k):
        return self.leaves('cell', None, k)

    def lattice(self, obj):
        return self.leaves('expr', obj, 0)


# -- assembled quantities -------------------------------------------------------------
def _part_degree(part, form_compiler_parameters=None):
    q = forms._quadrature_degree(part.metadata)
    if q is None:
        q = forms._quadrature_degree(form_compiler_parameters)
    return forms.check_degree(part.degree() if q is None else q)


def functional(form):
    '''assemble(form) of a rank-0 form or sum over dx and ds.'''
    total = 0.0
    with numpy.errstate(all='ignore'):
        for sign, part in form.terms():
            mesh = forms.form_mesh(part.integrand, part.mesh)
            q = _part_degree(part)
            if part.integral_type == 'cell':
                ctx = CellContext(mesh, q)
                v = evaluate(part.integrand.comps, ctx)
                total += sign * float(numpy.einsum(
                    'cq,q,c->', v, ctx.cells.wts, ctx.cells.adet))
            else:
                sel = facref.selection(mesh, part.subdomain_data,
                                       part.subdomain_id)
                ctx = FacetContext(mesh, q, sel)
                v = evaluate(part.integrand.comps, ctx)
                total += sign * float(numpy.einsum(
                    'mq,q,m->', v, ctx.F.wts, ctx.F.length))
    return total


def element_tensors(part, form_compiler_parameters=None):
    '''(V, Ke (Nc, nloc, nloc)) of a rank-2 part or (V, be (Nc, nloc)) of a
    rank-1 part, from the UNEXTRACTED integrand: basis functions stand for
    the arguments (bilinear_reference).'''
    V = part.arguments()[0]
    scheme = forms.quadrature_scheme(form_compiler_parameters, part.metadata)
    ctx = CellContext(V.mesh(), _part_degree(part, form_compiler_parameters),
                      scheme, V.degree)
    cells = ctx.cells
    nloc = V.layout.nloc
    nc = V.mesh().num_cells()
    tree = part.integrand.comps
    rank = len(forms.arguments(tree))
    scale = cells.wts[None, :] * cells.adet[:, None]
    with numpy.errstate(all='ignore'):
        if rank == 1:
            be = numpy.zeros((nc, nloc))
            for i in range(nloc):
                cells.index[0] = i
                be[:, i] = (evaluate(tree, ctx) * scale).sum(axis=1)
            return V, be
        Ke = numpy.zeros((nc, nloc, nloc))
        for i in range(nloc):
            for j in range(nloc):
                cells.index[0], cells.index[1] = i, j
                Ke[:, i, j] = (evaluate(tree, ctx) * scale).sum(axis=1)
    return V, Ke


def matrix(form, form_compiler_parameters=None):
    total = None
    for sign, part in form.terms():
        V, Ke = element_tensors(part, form_compiler_parameters)
        cd = V.layout.cell_dofs
        nloc = cd.shape[1]
        rows = numpy.repeat(cd, nloc, axis=1).reshape(-1)
        cols = numpy.tile(cd, (1, nloc)).reshape(-1)
        A = sp.coo_matrix((sign * Ke.reshape(-1), (rows, cols)),
                          shape=(V.N, V.N)).tocsr()
        total = A if total is None else total + A
    return total


def vector(form, form_compiler_parameters=None):
    total = None
    for sign, part in form.terms():
        V, be = element_tensors(part, form_compiler_parameters)
        b = numpy.zeros(V.N)
        numpy.add.at(b, V.layout.cell_dofs, sign * be)
        total = b if total is None else total + b
    return total


def point_values(expr, mesh, pts, cells):
    '''(components, n): the expression at located points.'''
    ctx = PointContext(mesh, pts, cells)
    with numpy.errstate(all='ignore'):
        return numpy.stack([evaluate(t, ctx) * numpy.ones(len(pts))
                            for t in fem.forms.as_form(expr).scalar_trees()])


def central_difference(F, u, w, eps):
    '''(F(u + eps w) - F(u - eps w)) / (2 eps) of a rank-1 form; u is
    restored.'''
    u0 = u.array().copy()
    u.set_array(u0 + eps * w)
    fp = vector(F)
    u.set_array(u0 - eps * w)
    fm = vector(F)
    u.set_array(u0)
    return (fp - fm) / (2.0 * eps)


# -- programs ---------------------------------------------------------------------------
def eval_tree(n, leaves):
    '''An argument-free scalar tree at the leaf values (newton_reference's
    eval_tree with the new nodes).'''
    with numpy.errstate(all='ignore'):
        return evaluate(n, LeafContext(leaves)) * numpy.ones(leaves.n)


def run_program(prog, leaves):
    '''{slot: values} of the instruction stream of a forms.Program: the
    register machine of csrc/form_kernels.hip in numpy, with the opcodes from
    19 up; the operations of the old opcodes are newton_reference's.'''
    names = {v: k for k, v in forms.OPS.items()}
    R = [None] * forms.REGISTERS
    out = {}
    with numpy.errstate(all='ignore'):
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
            elif name == 'cell':
                v = leaves('cell', None, a)
            elif name == 'mov':
                v = R[a]
            elif name == 'select':
                assert R[dst] is not None, 'select reads its destination'
                v = numpy.where(R[a] != 0.0, R[b], R[dst])
            elif name in _COMPARE:
                v = _COMPARE[name](R[a], R[b]).astype(float)
            elif name in _UNARY:
                v = _UNARY[name](R[a])
            else:
                v = _BINARY[name](R[a], R[b])
            assert v is not None, 'read of a register never written'
            assert 0 <= dst < forms.REGISTERS
            R[dst] = numpy.array(v, dtype=float)
    return out


# -- Newton on the host -------------------------------------------------------------------
def host_newton(F, u, bcs, J=None, maxit=50, rtol=1.0e-9, atol=1.0e-10,
                relax=1.0):
    '''newton_reference.host_newton with this module's matrices and vectors:
    (residual norms, iterations); the solution is left in u.'''
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
        A = K.dot(matrix(J)).dot(K) + sp.diags(1.0 - keep)
        b = keep * vector(F)
        res.append(float(numpy.linalg.norm(b)))
        if res[-1] < atol or res[-1] / res[0] < rtol or it == maxit:
            return res, it
        x = x - relax * spla.splu(A.tocsc()).solve(b)
        u.set_array(x)
        it += 1
