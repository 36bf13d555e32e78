# -*- coding: utf-8 -*-
'''
Forms of test and trial functions on a Taylor-Hood space WP (forms.py,
mixed_arguments): the reference's Stokes text

    (u, p) = TrialFunctions(WP); (v, q) = TestFunctions(WP)
    a = mu*inner(grad(u), grad(v))*dx - p*div(v)*dx - q*div(u)*dx
    L = inner(f, v)*dx
    A, b = assemble_system(a, L, bcs)

(flow/stokes.py:26-46) and its relatives with coefficients of the user's own:
a variable viscosity, a Brinkman insert alpha*dot(u, v)*dx(1), a penalty term
-eps*p*q*dx.  ops.assemble / ops.assemble_system / ops.solve hand forms whose
arguments live on a mixed space to this module.

The table of such a form has 3 x 3 blocks over the scalar components 0, 1
(velocity) and 2 (pressure) (forms.MixedTable).  Its velocity corner is the
BlockTable of a vector form and is assembled as one (ops._block_part:
flow_form_block_matrix / flow_form_block_vector), its pressure corner is the
table of a scalar form (flow_form_matrix / flow_form_vector), and the coupling
blocks -- a test function of one degree, a trial function of the other -- go
through flow_form_rect_matrix and its list forms over the rectangular pattern
of space.RectLayout.  Everything numerical is a call into libflow_hip.so.

Unknowns are numbered velocity x, velocity y, pressure: 2 Nv + Np.

solve(a == L, w, bcs) runs preconditioned MINRES (the loop of stokes._minres
over an abstract operator and preconditioner) and therefore takes SYMMETRIC
forms only; a non-symmetric mixed form is a NotImplementedError there -- there
is no flexible Krylov loop here that takes a block preconditioner yet --
while assemble_system and MixedMatrix.to_scipy() work for it.
'''
import ctypes

import numpy
import torch

from . import ops
from . import selection
from .function import Function, Vector
from .space import rect_layout
from .. import _hip
from .. import device


class RectMatrix(object):
    '''One value plane over a RectLayout: a rectangular kind-0 flow_operator
    (rows: dofs of the test layout, columns: dofs of the trial layout).'''

    def __init__(self, layout, vals=None):
        self.layout = layout
        self.shape = layout.shape
        # (readable past nnz: the SpMV loads value pairs)
        self.vals = device.zeros(layout.stride + 2) if vals is None else vals
        assert self.vals.numel() == layout.stride + 2
        assert self.vals.data_ptr() % 16 == 0
        self._op = None

    def plane(self):
        return self.vals[:self.layout.nnz]

    def operator(self):
        if self._op is None:
            lay = self.layout
            rb = lay.dev('rowblocks')
            op = _hip.Operator()
            op.kind = 0
            op.n = lay.shape[0]
            op.nnz = lay.nnz
            op.nblocks = rb.numel() - 1
            op.rowptr = _hip.i32(lay.dev('rowptr'), lay.shape[0] + 1, 'rowptr')
            op.cols = _hip.i32(lay.dev('cols'), lay.nnz, 'cols')
            op.rowblocks = _hip.i32(rb, None, 'rowblocks')
            op.vals[0] = _hip.f64(self.vals, lay.nnz, 'vals').value
            self._op = op
        return self._op

    def apply(self, x, y):
        _hip.check(_hip.lib().flow_operator_apply(
            ctypes.byref(self.operator()), _hip.f64(x, self.shape[1], 'x'),
            _hip.f64(y, self.shape[0], 'y'), _hip.stream()))
        return y

    def squared(self):
        '''The plane of the squared entries (the default pressure
        preconditioner's diag(B D^-1 B^T)).'''
        out = RectMatrix(self.layout)
        ops.vmul(self.vals, self.vals, out.vals)
        return out

    def to_scipy(self):
        import scipy.sparse as sp
        lay = self.layout
        v = device.to_host(self.vals).numpy()[:lay.nnz].copy()
        return sp.csr_matrix((v, lay.cols, lay.rowptr), shape=lay.shape)


class MixedMatrix(object):
    '''The matrix of a bilinear form on the Taylor-Hood space WP by blocks:
    uu, a kind-2 Matrix on the velocity layout; pp, a kind-0 Matrix on the
    pressure layout; up[r] (test component r, trial p) on RectLayout(kv, kp)
    and pu[s] (test q, trial component s) on RectLayout(kp, kv), RectMatrix
    planes -- the two planes of a pair share one pattern.  A block the form
    has no term for is None and costs nothing.'''

    def __init__(self, WP, uu=None, pp=None, up=None, pu=None):
        self.space = WP
        self.W, self.P = WP.taylor_hood()
        self.uu = uu
        self.pp = pp
        self.up = list(up) if up is not None else [None, None]
        self.pu = list(pu) if pu is not None else [None, None]
        self._tmp = None

    @property
    def size(self):
        return self.space.size()

    def blocks(self):
        '''[(name, block)] of the present blocks: 'uu', 'pp', 'up0', 'up1',
        'pu0', 'pu1'.'''
        named = [('uu', self.uu), ('pp', self.pp),
                 ('up0', self.up[0]), ('up1', self.up[1]),
                 ('pu0', self.pu[0]), ('pu1', self.pu[1])]
        return [(k, B) for k, B in named if B is not None]

    def apply(self, x, y):
        '''y = A x, composed of one flow_operator_apply per present block and
        an axpby where a second block lands on the same rows.'''
        assert x.data_ptr() != y.data_ptr()
        nv, n2 = self.W.N, self.W.size()
        npr = self.P.N
        assert x.numel() == self.size and y.numel() == self.size
        if self._tmp is None:
            self._tmp = device.empty(max(nv, npr))
        xu, xp, yu, yp = x[:n2], x[n2:], y[:n2], y[n2:]
        if self.uu is not None:
            self.uu.apply(xu, yu)
        else:
            _hip.fill(yu, 0.0)
        for r in range(2):
            if self.up[r] is not None:
                t = self._tmp[:nv]
                self.up[r].apply(xp, t)
                ops.axpby(1.0, t, 1.0, yu[r * nv:(r + 1) * nv])
        first = True
        if self.pp is not None:
            self.pp.apply(xp, yp)
            first = False
        for s in range(2):
            if self.pu[s] is None:
                continue
            xs = xu[s * nv:(s + 1) * nv]
            if first:
                self.pu[s].apply(xs, yp)
                first = False
            else:
                t = self._tmp[:npr]
                self.pu[s].apply(xs, t)
                ops.axpby(1.0, t, 1.0, yp)
        if first:
            _hip.fill(yp, 0.0)
        return y

    def __mul__(self, x):
        '''A * w for a Vector or a Function of WP: a new Vector.'''
        ops._no_strips('MixedMatrix * vector')
        data = x.data if isinstance(x, (Vector, Function)) else None
        if data is None:
            return NotImplemented
        if data.numel() != self.size:
            raise ValueError('matrix of size %d times a vector of %d entries'
                             % (self.size, data.numel()))
        return Vector(self.apply(data, device.empty(self.size)))

    __matmul__ = __mul__

    def to_scipy(self):
        '''One scipy.sparse CSR matrix in the numbering velocity x, velocity
        y, pressure, explicit zeros dropped.  Not for hot paths.'''
        import scipy.sparse as sp
        nv, npr = self.W.N, self.P.N
        uu = self.uu.to_scipy() if self.uu is not None \
            else sp.csr_matrix((2 * nv, 2 * nv))
        pp = self.pp.to_scipy() if self.pp is not None \
            else sp.csr_matrix((npr, npr))
        up = sp.vstack([B.to_scipy() if B is not None
                        else sp.csr_matrix((nv, npr)) for B in self.up])
        pu = sp.hstack([B.to_scipy() if B is not None
                        else sp.csr_matrix((npr, nv)) for B in self.pu])
        A = sp.bmat([[uu, up], [pu, pp]], format='csr')
        A.eliminate_zeros()
        A.sort_indices()
        return A


# -- assembly ---------------------------------------------------------------------
def rect_launch(R, part, fs, out):
    '''One program of a coupling block over the pattern R into the plane
    `out` (zero outside a ds / dx(k) part's targets): flow_form_rect_matrix,
    or its list form over the exterior facets / the cells of the part with
    the map of selection.rect_map.'''
    lib = _hip.lib()
    mesh = R.mesh
    nl2 = R.rows.nloc * R.cols_layout.nloc
    head = (ctypes.byref(ops.mesh_struct(mesh)),
            ctypes.byref(ops.space_struct(R.rows)),
            ctypes.byref(ops.space_struct(R.cols_layout)), ctypes.byref(fs))
    if part is None or (part.integral_type == 'cell'
                        and not ops.is_cell_subdomain(part)):
        n = nl2 * mesh.num_cells()
        _hip.check(lib.flow_form_rect_matrix(
            *head, _hip.f64(ops.scratch(mesh, n), n, 'scratch'),
            _hip.f64(out, R.nnz, 'vals'),
            _hip.i32(R.dev('cptr'), R.nnz + 1, 'cptr'),
            _hip.i32(R.dev('csrc'), n, 'csrc'), R.nnz, _hip.stream()))
        return
    cell = part.integral_type == 'cell'
    ops._list_launch(
        lib.flow_form_rect_cells_matrix if cell
        else lib.flow_form_rect_facet_matrix,
        head, mesh, *ops._selection_lists(mesh, part),
        selection.rect_map(R, cell, part.subdomain_data, part.subdomain_id),
        nl2, (out, R.nnz, 'vals'), (R.nnz,))


def _rect_part(part, block, q, scheme, R, mesh):
    '''One coupling block of one part into a fresh plane over R; a further
    program of the block into a plane of its own, then added.'''
    from . import forms
    facet = part.integral_type == 'exterior_facet'
    out = device.zeros(R.stride + 2)
    for k, prog in enumerate(forms.argument_programs(block, 2, facet)):
        fs, keep = ops._form_struct(prog, mesh, q, facet, scheme)
        dst = out if k == 0 else device.zeros(R.stride + 2)
        rect_launch(R, part, fs, dst)
        del keep
        if k:
            ops.axpby(1.0, dst, 1.0, out)
    return out


def assemble_form(form, rank, form_compiler_parameters=None):
    '''ops.assemble of a form (or signed sum) of arguments on a Taylor-Hood
    space: a MixedMatrix (rank 2) or a Vector of 2 Nv + Np (rank 1), part by
    part -- the programs of a part are compiled while the kernels of the part
    before run -- and, within a block, added in the order written.'''
    from . import forms
    if not forms.vector_arguments.enabled:
        raise NotImplementedError(
            'forms on a mixed space need vector_arguments(True) as well')
    WP = form.arguments()[0]
    W, P = WP.taylor_hood()
    mesh = WP.mesh()
    layv, layp = W.layout, P.layout
    Rup = rect_layout(mesh, W.degree, P.degree)
    Rpu = rect_layout(mesh, P.degree, W.degree)
    names = ['uu', 'pp'] + (['up0', 'up1', 'pu0', 'pu1'] if rank == 2 else [])
    sums = {k: ops._Sum() for k in names}
    for sign, part in form.terms():
        ops._check_part_mesh(part, mesh)
        _, table = part.argument_table()
        if not isinstance(table, forms.MixedTable):
            raise NotImplementedError(forms._MIXED_MISMATCH)
        q, scheme = ops._part_rule(part, form_compiler_parameters)
        corner = table.velocity()
        present = [b for row in corner for b in row] if rank == 2 \
            else list(corner)
        if any(b is not None for b in present):
            sums['uu'].add(sign, ops._block_part(part, corner, rank, q, scheme,
                                                 layv, mesh), True)
        pblock = table[2][2] if rank == 2 else table[2]
        if pblock is not None:
            ops._scalar_part(part, pblock, rank, q, scheme, layp, mesh,
                             sums['pp'], sign)
        if rank == 1:
            continue
        for c in range(2):
            if table[c][2] is not None:
                sums['up%d' % c].add(
                    sign, _rect_part(part, table[c][2], q, scheme, Rup, mesh),
                    True)
            if table[2][c] is not None:
                sums['pu%d' % c].add(
                    sign, _rect_part(part, table[2][c], q, scheme, Rpu, mesh),
                    True)
    if all(s.total is None for s in sums.values()):
        raise ValueError('an empty sum of forms has no rank')
    if rank == 1:
        out = device.zeros(WP.size())
        if sums['uu'].total is not None:
            _hip.copy(out[:W.size()], sums['uu'].total)
        if sums['pp'].total is not None:
            _hip.copy(out[W.size():], sums['pp'].total)
        return Vector(out)
    tot = {k: s.total for k, s in sums.items()}
    return MixedMatrix(
        WP,
        None if tot['uu'] is None else ops.Matrix(layv, 2, tot['uu']),
        None if tot['pp'] is None else ops.Matrix(layp, 0, tot['pp']),
        [None if tot['up%d' % r] is None else RectMatrix(Rup, tot['up%d' % r])
         for r in range(2)],
        [None if tot['pu%d' % s] is None else RectMatrix(Rpu, tot['pu%d' % s])
         for s in range(2)])


# -- the symmetric part -------------------------------------------------------------
def _transpose_perm(lay, other=None):
    '''The device permutation that takes the entries of the pattern `lay` (a
    ScalarLayout, or a RectLayout with `other` the layout of the transposed
    block) to their mirror images; held on the layout.'''
    from .space import transpose_permutation
    if 'transpose_perm' not in lay._dev:
        if other is None:
            rp, cols = lay.pattern('rowptr'), lay.pattern('cols')
            perm = transpose_permutation(rp, cols, rp, cols)
        else:
            perm = transpose_permutation(lay.rowptr, lay.cols, other.rowptr,
                                         other.cols)
        lay._dev['transpose_perm'] = device.to_device(perm)
    return lay._dev['transpose_perm']


def _symmetric_part(a, b, nb, perm, n, out):
    _hip.check(_hip.lib().flow_plane_symmetric_part(
        n, _hip.f64(a, n, 'a'), _hip.f64(b, nb, 'b'), nb,
        _hip.i32(perm, n, 'perm'), _hip.f64(out, n, 'out'), _hip.stream()))


def symmetric_part(A):
    '''(A + A^T) / 2 of a MixedMatrix, block by block (flow_plane_symmetric_
    part): mirrored entries hold the same bits.  The element kernels give
    entry (i, j) as (w c dpsi_j) dphi_i and entry (j, i) as (w c dphi_i)
    dpsi_j, which differ in the last bit, so the assembled matrix of a
    symmetric form is symmetric to rounding only; assemble_system returns
    this part for a structurally symmetric form, which moves no entry by more
    than that rounding.  A coupling block whose mirror block is absent is a
    ValueError: such a matrix does not come from a symmetric form.'''
    uu = pp = None
    if A.uu is not None:
        lay, st = A.uu.layout, A.uu.stride
        perm = _transpose_perm(lay)
        uu = ops.Matrix(lay, 2)
        for r in range(2):
            for s in range(2):
                p, t = 2 * r + s, 2 * s + r
                _symmetric_part(A.uu.vals[p * st:], A.uu.vals[t * st:],
                                lay.nnz, perm, lay.nnz, uu.vals[p * st:])
    if A.pp is not None:
        lay = A.pp.layout
        pp = ops.Matrix(lay, 0)
        _symmetric_part(A.pp.vals, A.pp.vals, lay.nnz, _transpose_perm(lay),
                        lay.nnz, pp.vals)
    up, pu = [None, None], [None, None]
    for c in range(2):
        B, C = A.up[c], A.pu[c]
        if B is None and C is None:
            continue
        if B is None or C is None:
            raise ValueError('symmetric_part: coupling block %d has no mirror '
                             'block' % c)
        Rup, Rpu = B.layout, C.layout
        up[c], pu[c] = RectMatrix(Rup), RectMatrix(Rpu)
        _symmetric_part(B.vals, C.vals, Rpu.nnz, _transpose_perm(Rup, Rpu),
                        Rup.nnz, up[c].vals)
        _symmetric_part(C.vals, B.vals, Rup.nnz, _transpose_perm(Rpu, Rup),
                        Rpu.nnz, pu[c].vals)
    return MixedMatrix(A.space, uu, pp, up, pu)


# -- Dirichlet conditions -----------------------------------------------------------
def mixed_bcs(bcs, WP):
    '''(dofs, values, velocity mask of 2 Nv bytes, pressure mask of Np bytes)
    of conditions on WP.sub(0), WP.sub(0).sub(i) and WP.sub(1), dofs in the
    numbering velocity x, velocity y, pressure; host arrays, None without any
    condition.  A condition on any other space is the ValueError of
    ops._scalar_bcs.'''
    from .bcs import collect
    W, P = WP.taylor_hood()
    if bcs is None:
        bcs = []
    if not isinstance(bcs, (list, tuple)):
        bcs = [bcs]
    ubcs, pbcs = [], []
    for bc in bcs:
        S = bc.function_space()
        T = S.parent if getattr(S, 'component', None) is not None else S
        if T is not None and W.same_as(T):
            ubcs.append(bc)
        elif getattr(S, 'component', 0) is None and P.same_as(S):
            pbcs.append(bc)
        else:
            raise ValueError('a Dirichlet condition lives on another space '
                             'than the form')
    ud, uv = collect(ubcs, W.size())
    pd, pv = collect(pbcs, P.size())
    if len(ud) + len(pd) == 0:
        return None
    umask = numpy.zeros(W.size(), dtype=numpy.uint8)
    umask[ud] = 1
    pmask = numpy.zeros(P.size(), dtype=numpy.uint8)
    pmask[pd] = 1
    dofs = numpy.concatenate([ud, pd + W.size()]).astype(numpy.int32)
    return dofs, numpy.concatenate([uv, pv]), umask, pmask


def _rect_mask(B, row_isbc, col_isbc):
    lay = B.layout
    _hip.check(_hip.lib().flow_bc_rect_mask(
        _hip.i32(lay.dev('rowptr'), lay.shape[0] + 1, 'rowptr'),
        _hip.i32(lay.dev('cols'), lay.nnz, 'cols'), lay.shape[0],
        _hip.f64(B.vals, lay.nnz, 'vals'),
        _hip.u8(row_isbc, lay.shape[0], 'row_isbc'),
        _hip.u8(col_isbc, lay.shape[1], 'col_isbc'), _hip.stream()))
    return B


def assemble_system(a, L, bcs=None, form_compiler_parameters=None,
                    masks=None):
    '''(A, b) of a bilinear and a linear form on a Taylor-Hood space with
    dolfin's symmetric elimination.  The matrix of a structurally symmetric
    form (forms.is_symmetric_form) is first replaced by its symmetric part
    (symmetric_part: the kernels' (i, j) and (j, i) entries differ in the last
    bit), so that A is symmetric bit for bit.  Then b -= A g, b[dof] = g, and
    symmetric_bc_blocks on uu, symmetric_bc_matrix on pp (a pressure
    condition without a pp term makes pp an explicit matrix with unit diagonal
    on the condition's rows) and flow_bc_rect_mask on the coupling planes.
    masks: a dict that receives the host masks 'u' and 'p' (solve's
    preconditioner reads them).'''
    from . import forms
    WP = a.arguments()[0]
    W, P = WP.taylor_hood()
    A0 = ops.assemble(a, form_compiler_parameters)
    if forms.is_symmetric_form(a):
        # (bit for bit symmetric, as dolfin's assemble_system keeps a
        # symmetric form's matrix: MINRES relies on it)
        A0 = symmetric_part(A0)
    if L is None or (isinstance(L, forms.FormSum) and not L.terms()):
        b = Vector(device.zeros(WP.size()))
    else:
        if L.rank != 1:
            raise ValueError('the right-hand side must be a linear form '
                             '(rank 1)')
        if not forms._same_space(L.arguments()[0], WP):
            raise NotImplementedError('test functions of different spaces or '
                                      'meshes on the two sides')
        b = ops.assemble(L, form_compiler_parameters)
    held = mixed_bcs(bcs, WP)
    if masks is not None:
        masks['u'] = None if held is None else held[2]
        masks['p'] = None if held is None else held[3]
    if held is None:
        return A0, b
    dofs, vals, umask, pmask = held
    nv = W.N
    ddofs, dvals = device.to_device(dofs), device.to_device(vals)
    g = device.zeros(WP.size())
    ops._set_values(ddofs, dvals, g)
    lift = A0.apply(g, device.empty(WP.size()))
    ops.axpby(-1.0, lift, 1.0, b.data)
    ops._set_values(ddofs, dvals, b.data)
    um, pm = device.to_device(umask), device.to_device(pmask)
    uu = A0.uu
    if uu is None and umask.any():
        uu = ops.Matrix(W.layout, 2)
    if uu is not None:
        uu = ops.symmetric_bc_blocks(uu, um)
    pp = A0.pp
    if pp is None and pmask.any():
        pp = ops.Matrix(P.layout, 0)
    if pp is not None:
        pp = ops.symmetric_bc_matrix(pp, pm)
    ums = [um[r * nv:(r + 1) * nv].contiguous() for r in range(2)]
    up = [None if B is None else _rect_mask(B, ums[r], pm)
          for r, B in enumerate(A0.up)]
    pu = [None if B is None else _rect_mask(B, pm, ums[s])
          for s, B in enumerate(A0.pu)]
    return MixedMatrix(WP, uu, pp, up, pu), b


# -- MINRES ---------------------------------------------------------------------------
def minres(apply_A, precondition, b, x, rtol, atol=0.0, maxit=1000):
    '''Preconditioned MINRES (Paige & Saunders; Elman, Silvester & Wathen,
    Alg. 4.1) for a symmetric operator and a symmetric positive definite
    preconditioner: the loop of stokes._minres over apply_A(x, y) and
    precondition(v, z) on device vectors of one length.  x holds the initial
    guess and receives the solution.  Converged when the preconditioned
    residual norm has fallen below max(rtol * its initial value, atol).
    Host-looped: two dots per iteration are read back.  Returns
    (iterations, preconditioned residual norm); raises _hip.NotConverged.'''
    n = b.numel()
    new = lambda: device.zeros(n)   # noqa: E731
    v_old, v, v_new = new(), new(), new()
    z, z_new = new(), new()
    w_old, w, w_new = new(), new(), new()
    Az = new()
    # v = b - A x0
    apply_A(x, Az)
    ops.copy(v, b)
    ops.axpby(-1.0, Az, 1.0, v)
    precondition(v, z)
    gamma = numpy.sqrt(max(ops.dot(z, v), 0.0))
    gamma0 = gamma
    eta = gamma
    s_old = s_cur = 0.0
    c_old = c_cur = 1.0
    gamma_old = 1.0
    its = 0
    res = gamma
    while gamma0 > 0.0 and abs(res) > max(rtol * gamma0, atol):
        if its >= maxit:
            raise _hip.NotConverged(
                'MINRES did not converge in %d iterations (|r|/|r0| = %.3e > '
                '%.3e)' % (its, abs(res) / gamma0, rtol))
        ops.axpby(0.0, z, 1.0 / gamma, z)
        apply_A(z, Az)
        delta = ops.dot(Az, z)
        ops.copy(v_new, Az)
        ops.axpby(-delta / gamma, v, 1.0, v_new)
        if its > 0:
            ops.axpby(-gamma / gamma_old, v_old, 1.0, v_new)
        precondition(v_new, z_new)
        gamma_new = numpy.sqrt(max(ops.dot(z_new, v_new), 0.0))
        a0 = c_cur * delta - c_old * s_cur * gamma
        a1 = numpy.sqrt(a0 * a0 + gamma_new * gamma_new)
        a2 = s_cur * delta + c_old * c_cur * gamma
        a3 = s_old * gamma
        c_new, s_new = a0 / a1, gamma_new / a1
        ops.copy(w_new, z)
        ops.axpby(-a3, w_old, 1.0, w_new)
        ops.axpby(-a2, w, 1.0, w_new)
        ops.axpby(0.0, w_new, 1.0 / a1, w_new)
        ops.axpby(c_new * eta, w_new, 1.0, x)
        eta = -s_new * eta
        res = eta
        v_old, v, v_new = v, v_new, v_old
        z, z_new = z_new, z
        w_old, w, w_new = w, w_new, w_old
        gamma_old, gamma = gamma, gamma_new
        s_old, s_cur = s_cur, s_new
        c_old, c_cur = c_cur, c_new
        its += 1
        if gamma == 0.0:
            break
    return its, abs(res)


class BlockPreconditioner(object):
    '''blockdiag(velocity part, inverse of a positive pressure diagonal) for
    MINRES on an eliminated MixedMatrix A.  velocity 'jacobi': the inverse
    diagonal of uu; 'two_level': flow_two_level_apply with one ops.CoarseSpace
    per diagonal plane of uu, as stokes._minres does -- every velocity
    component then needs a Dirichlet dof (ValueError otherwise).  pdiag: the pressure
    diagonal on the device (Dirichlet rows 1).  Dirichlet rows are identity:
    the eliminated uu has a unit diagonal there, and its coarse spaces leave
    those dofs out.'''

    def __init__(self, A, velocity, pdiag, umask):
        if velocity not in ('jacobi', 'two_level'):
            raise ValueError("preconditioner %r: 'jacobi' or 'two_level'"
                             % (velocity,))
        if A.uu is None:
            raise ValueError('the form has no velocity-velocity block: '
                             'nothing to precondition the velocity with')
        self.A = A
        self.velocity = velocity
        self.nv, self.n2 = A.W.N, A.W.size()
        self.dinv = A.uu.diag_inv()
        self.minv = torch.reciprocal(pdiag)
        if velocity == 'two_level':
            lay = A.W.layout
            nv = self.nv
            self.coarse = []
            for c in range(2):
                p = 3 * c
                plane = ops.Matrix(lay, 0, A.uu.vals[
                    p * A.uu.stride:(p + 1) * A.uu.stride].clone())
                isbc = None if umask is None else umask[c * nv:(c + 1) * nv]
                if isbc is None or not isbc.any():
                    # (whether that plane is singular -- a pure Laplacian --
                    # or not -- a mass or Brinkman term -- is not known here,
                    # and the coarse inverse must fit: MINRES needs a positive
                    # definite preconditioner)
                    raise ValueError(
                        "preconditioner 'two_level' needs a Dirichlet "
                        'condition on every velocity component (component %d '
                        "has none): use 'jacobi'" % c)
                self.coarse.append(ops.CoarseSpace(plane, isbc, False))
            self.cwork = device.empty(
                2 * max(c.struct.lda for c in self.coarse) + 2)

    def apply(self, v, z):
        n2, nv = self.n2, self.nv
        if self.velocity == 'jacobi':
            ops.vmul(v[:n2], self.dinv, z[:n2])
        else:
            lib = _hip.lib()
            for c in range(2):
                sl = slice(c * nv, (c + 1) * nv)
                _hip.check(lib.flow_two_level_apply(
                    ctypes.byref(self.coarse[c].struct),
                    _hip.f64(self.dinv[sl], nv), _hip.f64(v[sl], nv),
                    _hip.f64(z[sl], nv), _hip.f64(self.cwork), _hip.stream()))
        ops.vmul(v[n2:], self.minv, z[n2:])
        return z


def _schur_diagonal(A, pmask):
    '''diag(B diag(uu)^-1 B^T) of the eliminated A: the squared coupling
    planes pu[s] applied to uu.diag_inv(), summed; rows without an entry and
    Dirichlet rows 1.'''
    nv, npr = A.W.N, A.P.N
    dinv = A.uu.diag_inv()
    d = device.zeros(npr)
    tmp = device.empty(npr)
    for s in range(2):
        if A.pu[s] is None:
            continue
        A.pu[s].squared().apply(dinv[s * nv:(s + 1) * nv], tmp)
        ops.axpby(1.0, tmp, 1.0, d)
    d = torch.abs(d)
    one = torch.ones_like(d)
    d = torch.where(d > 0.0, d, one)
    if pmask is not None:
        d = torch.where(device.to_device(pmask) != 0, one, d)
    return d


def _form_diagonal(prec_form, bcs, form_compiler_parameters):
    '''The absolute lumped rows of the pp block of a rank-2 mixed form (the
    reference's mu*inner(grad(u), grad(v))*dx - p*q*dx idiom; its sign is
    ignored), eliminated with the same conditions: Dirichlet rows 1.'''
    M, _ = assemble_system(prec_form, None, bcs, form_compiler_parameters)
    if M.pp is None:
        raise ValueError("'preconditioner_form' has no pressure-pressure "
                         'term (p*q*dx) to precondition the pressure with')
    npr = M.P.N
    d = torch.abs(M.pp.apply(device.zeros(npr) + 1.0, device.empty(npr)))
    if not bool((d > 0.0).all()):
        raise ValueError("'preconditioner_form': a lumped pressure row is "
                         'zero')
    return d


def solve(a, L, w, bcs=None, solver_parameters=None,
          form_compiler_parameters=None):
    '''solve(a == L, w, bcs) with w = Function(WP): assemble_system, then
    preconditioned MINRES from w's values into w.  The form must be symmetric
    -- structurally (forms.is_symmetric_form: over all its parts) or by
    solver_parameters['symmetric'] = True --, else NotImplementedError: there
    is no flexible Krylov loop that takes a block preconditioner yet
    (assemble_system and to_scipy() still work for such a form).
    A structurally symmetric form is solved on the bitwise symmetric matrix
    of assemble_system; a form that only 'symmetric': True vouches for is NOT
    symmetrised (its blocks need not have mirror blocks), so MINRES then runs
    on an operator that is symmetric to rounding only.
    solver_parameters: 'preconditioner' 'jacobi' (default) | 'two_level' for
    the velocity part ('two_level': a Dirichlet dof on every velocity
    component); 'preconditioner_form', a rank-2 mixed form whose pp
    block's absolute lumped rows precondition the pressure (default:
    diag(B diag(uu)^-1 B^T)); 'krylov_solver': 'relative_tolerance' (1e-12,
    on the preconditioned residual), 'absolute_tolerance' (0),
    'maximum_iterations' (1000).  A singular pressure (all-Dirichlet velocity,
    nothing pinned) is the user's to pin.  Returns an ops.SolveInfo; raises
    _hip.NotConverged.'''
    from . import forms
    WP = a.arguments()[0]
    if not isinstance(w, Function) or not forms.is_mixed_space(
            w.function_space()) or not w.function_space().same_as(WP):
        raise ValueError('solve writes into a Function of the space of the '
                         'trial function')
    prm = dict(solver_parameters or {})
    symmetric = prm.get('symmetric') is True or forms.is_symmetric_form(a)
    if not symmetric:
        raise NotImplementedError(
            'solve of a non-symmetric form on a mixed space: MINRES needs a '
            'symmetric form, and there is no flexible Krylov loop that takes '
            'a block preconditioner yet; assemble_system(a, L, bcs) and '
            'to_scipy() work for it')
    ks = dict(prm.get('krylov_solver') or {})
    masks = {}
    A, b = assemble_system(a, L, bcs, form_compiler_parameters, masks)
    if prm.get('preconditioner_form') is not None:
        pdiag = _form_diagonal(prm['preconditioner_form'], bcs,
                               form_compiler_parameters)
    else:
        if A.uu is None:
            raise ValueError('the form has no velocity-velocity block')
        pdiag = _schur_diagonal(A, masks['p'])
    M = BlockPreconditioner(A, prm.get('preconditioner', 'jacobi'), pdiag,
                            masks['u'])
    its, res = minres(A.apply, M.apply, b.data, w.data,
                      ks.get('relative_tolerance', 1.0e-12),
                      ks.get('absolute_tolerance', 0.0),
                      int(ks.get('maximum_iterations', 1000)))
    return ops.SolveInfo(its, res, 'minres')
