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
over an abstract operator and preconditioner) for SYMMETRIC forms.  A
non-symmetric mixed form (Oseen, a Picard step of Navier-Stokes, +q*div(u))
is a NotImplementedError unless forms.mixed_gmres(True) is on: then it runs
right-preconditioned flexible GMRES (fgmres) with a block-triangular
preconditioner (BlockTriangularPreconditioner: ILU(0) or Jacobi on uu, a
signed approximate Schur diagonal on the pressure) over the product of all
blocks in one launch (MixedMatrix.apply_fused: flow_mixed_apply, csrc/
mixed_kernels.hip).  assemble_system and MixedMatrix.to_scipy() work for such
a form either way.

With forms.mixed_derivatives(True), solve(F == 0, w, bcs) on WP is Newton's
method (newton_solve): MixedNewtonAssembler holds J = derivative(F, w) and F,
assembles the blocks of J that do not read w once, and every step solves
J delta = F by fgmres over apply_fused with the block-triangular preconditioner
whose first half runs in one launch (BlockTriangularPreconditioner.
apply_fused: flow_mixed_upper_rhs).
'''
import ctypes

import numpy
import torch

from . import ops
from . import selection
from .function import Function, Vector
from .space import rect_layout, csr_stream_rowblocks
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
        self._fused = None

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

    def fused(self):
        '''The flow_mixed struct of the present blocks (include/flow_hip.h)
        with the velocity and pressure tiles of fused_tiles; cached.'''
        if self._fused is None:
            mesh = self.space.mesh()
            layv, layp = self.W.layout, self.P.layout
            Rup = rect_layout(mesh, self.W.degree, self.P.degree)
            Rpu = rect_layout(mesh, self.P.degree, self.W.degree)
            vt, pt = fused_tiles(Rup, True), fused_tiles(Rpu, True)
            s = _hip.MixedS()
            s.nv, s.np = layv.N, layp.N
            s.nvtiles, s.nptiles = vt.numel() - 1, pt.numel() - 1
            s.vtiles = _hip.i32(vt, None, 'vtiles')
            s.ptiles = _hip.i32(pt, None, 'ptiles')
            s.vrowptr = _hip.i32(layv.dev('rowptr'), layv.N + 1, 'rowptr')
            s.vcols = _hip.i32(layv.dev('cols'), layv.nnz, 'cols')
            s.prowptr = _hip.i32(layp.dev('rowptr'), layp.N + 1, 'rowptr')
            s.pcols = _hip.i32(layp.dev('cols'), layp.nnz, 'cols')
            s.uprowptr = _hip.i32(Rup.dev('rowptr'), layv.N + 1, 'rowptr')
            s.upcols = _hip.i32(Rup.dev('cols'), Rup.nnz, 'cols')
            s.purowptr = _hip.i32(Rpu.dev('rowptr'), layp.N + 1, 'rowptr')
            s.pucols = _hip.i32(Rpu.dev('cols'), Rpu.nnz, 'cols')
            if self.uu is not None:
                assert self.uu.kind == 2 and self.uu.layout is layv
                for p in range(4):
                    s.uu[p] = self.uu.operator().vals[p]
            if self.pp is not None:
                assert self.pp.kind == 0 and self.pp.layout is layp
                s.pp = self.pp.operator().vals[0]
            for c in range(2):
                if self.up[c] is not None:
                    assert self.up[c].layout is Rup
                    s.up[c] = self.up[c].operator().vals[0]
                if self.pu[c] is not None:
                    assert self.pu[c].layout is Rpu
                    s.pu[c] = self.pu[c].operator().vals[0]
            self._fused = s
        return self._fused

    def apply_fused(self, x, y):
        '''y = A x in one launch (flow_mixed_apply): every entry has the bits
        apply() leaves there.  y overlapping x is a ValueError.'''
        assert x.numel() == self.size and y.numel() == self.size
        _hip.check(_hip.lib().flow_mixed_apply(
            ctypes.byref(self.fused()), _hip.f64(x, self.size, 'x'),
            _hip.f64(y, self.size, 'y'), _hip.stream()))
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


def _tile_cap():
    '''Nonzeros a tile of flow_mixed_apply may hold in each of its patterns:
    the caps of the CSR-stream kernels of kind 0 and kind 2 (the header's
    constant without a built library).'''
    try:
        return min(_hip.spmv_tile_nnz(0), _hip.spmv_tile_nnz(2))
    except (OSError, _hip.HipError):
        return _hip.SPMV_NNZ_PER_BLOCK


def fused_tiles(R, dev=False):
    '''Row tiles of flow_mixed_apply over the rows of the RectLayout R: at
    most 256 consecutive rows that stay within the tile cap both in the
    square pattern of R's row layout and in R's own -- the velocity tiles for
    R = RectLayout(kv, kp), the pressure tiles for RectLayout(kp, kv).  Held
    on R (dev: the device copy).'''
    if 'mixed_tiles_host' not in R._dev:
        R._dev['mixed_tiles_host'] = csr_stream_rowblocks(
            [R.rows.pattern('rowptr'), R.rowptr], nnz_per_block=_tile_cap())
    if not dev:
        return R._dev['mixed_tiles_host']
    if 'mixed_tiles' not in R._dev:
        R._dev['mixed_tiles'] = device.to_device(R._dev['mixed_tiles_host'])
    return R._dev['mixed_tiles']


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


def assemble_form(form, rank, form_compiler_parameters=None, only=None):
    '''ops.assemble of a form (or signed sum) of arguments on a Taylor-Hood
    space: a MixedMatrix (rank 2) or a Vector of 2 Nv + Np (rank 1), part by
    part -- the programs of a part are compiled while the kernels of the part
    before run -- and, within a block, added in the order written.  only: the
    names of the blocks to assemble (MixedMatrix.blocks() naming; the others
    come out absent) -- a block's launches and sum do not depend on the
    others, so it has the bits it has in the whole matrix
    (MixedNewtonAssembler skips its frozen blocks so).'''
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
    want = (lambda k: True) if only is None else (lambda k: k in only)
    for sign, part in form.terms():
        ops._check_part_mesh(part, mesh)
        _, table = part.argument_table()
        if not isinstance(table, forms.MixedTable):
            raise NotImplementedError(forms._MIXED_MISMATCH)
        q, scheme = ops._part_rule(part, form_compiler_parameters)
        corner = table.velocity()
        present = [b for row in corner for b in row] if rank == 2 \
            else list(corner)
        if want('uu') and any(b is not None for b in present):
            sums['uu'].add(sign, ops._block_part(part, corner, rank, q, scheme,
                                                 layv, mesh), True)
        pblock = table[2][2] if rank == 2 else table[2]
        if want('pp') and pblock is not None:
            ops._scalar_part(part, pblock, rank, q, scheme, layp, mesh,
                             sums['pp'], sign)
        if rank == 1:
            continue
        for c in range(2):
            if want('up%d' % c) and table[c][2] is not None:
                sums['up%d' % c].add(
                    sign, _rect_part(part, table[c][2], q, scheme, Rup, mesh),
                    True)
            if want('pu%d' % c) and table[2][c] is not None:
                sums['pu%d' % c].add(
                    sign, _rect_part(part, table[2][c], q, scheme, Rpu, mesh),
                    True)
    if only is None and all(s.total is None for s in sums.values()):
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


def _form_diagonal(prec_form, bcs, form_compiler_parameters, signed=False):
    '''The absolute lumped rows of the pp block of a rank-2 mixed form (the
    reference's mu*inner(grad(u), grad(v))*dx - p*q*dx idiom; its sign is
    ignored), eliminated with the same conditions: Dirichlet rows 1.
    signed (the GMRES path): the lumped rows as written, with their sign.'''
    M, _ = assemble_system(prec_form, None, bcs, form_compiler_parameters)
    if M.pp is None:
        raise ValueError("'preconditioner_form' has no pressure-pressure "
                         'term (p*q*dx) to precondition the pressure with')
    npr = M.P.N
    d = M.pp.apply(device.zeros(npr) + 1.0, device.empty(npr))
    if not bool((torch.abs(d) > 0.0).all()):
        raise ValueError("'preconditioner_form': a lumped pressure row is "
                         'zero')
    return d if signed else torch.abs(d)


# -- flexible GMRES ---------------------------------------------------------------
def fgmres(apply_A, precondition, b, x, rtol, atol=0.0, maxit=1000,
           restart=30):
    '''Right-preconditioned flexible GMRES(restart) (Saad, Alg. 9.6) over
    apply_A(x, y) and precondition(v, z) on device vectors of one length: the
    preconditioned vectors Z_j are kept and x is updated from them, as
    flow_gmres_solve does, so the preconditioner may change from one
    application to the next (sweeps in reduced precision).  x holds the
    initial guess and receives the solution.
    Host-looped.  The basis V and Z are column-major device stores with an
    even leading dimension (16-byte aligned columns); an Arnoldi step
    orthogonalises by classical Gram-Schmidt with a second pass: per pass one
    flow_multi_dot launch over the basis and one read-back, and one
    flow_combine for the subtraction; one more dot gives the norm.  Givens
    rotations run on the host.
    Stopping: within a cycle the rotated residual estimate is watched; at a
    restart and on exit the TRUE residual |b - A x|_2 is computed and tested
    against max(rtol |b|_2, atol), flow_gmres_solve's rule for right
    preconditioning.  Every kernel has a fixed summation order: the same call
    gives the same bits.  Returns (iterations, true residual norm); raises
    _hip.NotConverged.'''
    lib = _hip.lib()
    n = b.numel()
    m = max(1, int(restart))
    ld = n + (n & 1)
    V = device.zeros((m + 1) * ld)
    Z = device.zeros(m * ld)
    assert V.data_ptr() % 16 == 0 and Z.data_ptr() % 16 == 0
    col = lambda S, j: S[j * ld:j * ld + n]   # noqa: E731
    w, w1 = device.zeros(n), device.zeros(n)
    dwork = device.empty((m + 1) * _hip.MULTI_DOT_BLOCKS)
    dots = device.empty(m + 1)

    def project(k, y, out):
        '''out = y - V[:, :k] (V[:, :k]^T y); returns the k coefficients.'''
        _hip.check(lib.flow_multi_dot(
            n, k, _hip.f64(V, (k - 1) * ld + n, 'basis'), ld,
            _hip.f64(y, n, 'y'), _hip.f64(dwork, k * _hip.MULTI_DOT_BLOCKS),
            _hip.f64(dots, k), _hip.stream()))
        h = device.to_host(dots[:k]).numpy().astype(numpy.float64)
        combine(V, k, -h, y, out)
        return h

    def combine(S, k, coef, base, out):
        '''out = base + S[:, :k] coef (flow_combine; out overlaps nothing).'''
        C = device.to_device(numpy.ascontiguousarray(coef, numpy.float64))
        _hip.check(lib.flow_combine(
            n, k, _hip.f64(S, (k - 1) * ld + n, 'columns'), ld, 1,
            _hip.f64(C, k, 'coefficients'), _hip.f64(base, n, 'base'),
            _hip.f64(out, n, 'out'), ld, _hip.stream()))

    def residual(dst):
        apply_A(x, w)
        ops.copy(dst, b)
        ops.axpby(-1.0, w, 1.0, dst)
        return numpy.sqrt(max(ops.dot(dst, dst), 0.0))

    tol = max(rtol * numpy.sqrt(max(ops.dot(b, b), 0.0)), atol)
    its = 0
    beta = residual(col(V, 0))
    while beta > tol:
        if its >= maxit:
            raise _hip.NotConverged(
                'FGMRES did not converge in %d iterations (|b - A x| = %.3e > '
                '%.3e)' % (its, beta, tol))
        ops.axpby(0.0, col(V, 0), 1.0 / beta, col(V, 0))
        H = numpy.zeros((m + 1, m))
        g = numpy.zeros(m + 1)
        g[0] = beta
        cs, sn = numpy.zeros(m), numpy.zeros(m)
        k = 0
        while k < m and its < maxit:
            j = k
            precondition(col(V, j), col(Z, j))
            apply_A(col(Z, j), w)
            h = project(j + 1, w, w1)
            h = h + project(j + 1, w1, col(V, j + 1))
            vn = col(V, j + 1)
            hn = numpy.sqrt(max(ops.dot(vn, vn), 0.0))
            H[:j + 1, j] = h
            H[j + 1, j] = hn
            for i in range(j):
                t = cs[i] * H[i, j] + sn[i] * H[i + 1, j]
                H[i + 1, j] = -sn[i] * H[i, j] + cs[i] * H[i + 1, j]
                H[i, j] = t
            d = numpy.hypot(H[j, j], H[j + 1, j])
            if d == 0.0:
                break    # (A Z_j lies in the span and adds nothing: singular)
            cs[j], sn[j] = H[j, j] / d, H[j + 1, j] / d
            H[j, j], H[j + 1, j] = d, 0.0
            g[j + 1] = -sn[j] * g[j]
            g[j] = cs[j] * g[j]
            k += 1
            its += 1
            if hn == 0.0 or abs(g[k]) <= tol:
                break
            ops.axpby(0.0, vn, 1.0 / hn, vn)
        if k == 0:
            raise _hip.NotConverged(
                'FGMRES broke down after %d iterations (|b - A x| = %.3e > '
                '%.3e)' % (its, beta, tol))
        y = numpy.zeros(k)
        for i in range(k - 1, -1, -1):
            y[i] = (g[i] - H[i, i + 1:k].dot(y[i + 1:])) / H[i, i]
        combine(Z, k, y, x, w1)
        ops.copy(x, w1)
        beta = residual(col(V, 0))
    return its, beta


class BlockTriangularPreconditioner(object):
    '''The block upper triangular preconditioner [[F~, up], [0, diag(sdiag)]]
    of an eliminated MixedMatrix A for fgmres:
        z_p = r_p / sdiag;  z_u = F~^-1 (r_u - up z_p).
    velocity 'ilu0' (default): one application of Ilu0(A.uu), the ILU(0)
    factors of the two diagonal planes of uu; 'jacobi': A.uu.diag_inv().
    sdiag: the signed approximate Schur diagonal on the device
    (_signed_schur_diagonal, or the lumped rows of a preconditioner form),
    Dirichlet rows 1.  Dirichlet rows are identity rows: the eliminated uu has
    unit rows there and the coupling planes are zero on them.'''

    def __init__(self, A, velocity='ilu0', sdiag=None):
        if velocity not in ('ilu0', 'jacobi'):
            raise ValueError("preconditioner %r under GMRES: 'ilu0' or "
                             "'jacobi'" % (velocity,))
        if A.uu is None:
            raise ValueError('the form has no velocity-velocity block: '
                             'nothing to precondition the velocity with')
        from .ilu import Ilu0
        self.A = A
        self.velocity = velocity
        self.nv, self.n2 = A.W.N, A.W.size()
        if sdiag is None:
            sdiag = _signed_schur_diagonal(A, None)
        self.sinv = torch.reciprocal(sdiag)
        self.ru = device.empty(self.n2)
        self.tmp = device.empty(self.nv)
        if velocity == 'ilu0':
            self.ilu = Ilu0(A.uu)
            self.work = device.empty(self.n2)
        else:
            self.dinv = A.uu.diag_inv()

    def apply(self, v, z):
        n2, nv = self.n2, self.nv
        zp = z[n2:]
        ops.vmul(v[n2:], self.sinv, zp)
        ru = ops.copy(self.ru, v[:n2])
        for r in range(2):
            if self.A.up[r] is not None:
                self.A.up[r].apply(zp, self.tmp)
                ops.axpby(-1.0, self.tmp, 1.0, ru[r * nv:(r + 1) * nv])
        if self.velocity == 'jacobi':
            ops.vmul(ru, self.dinv, z[:n2])
        else:
            _hip.check(_hip.lib().flow_ilu0_solve(
                ctypes.byref(self.ilu.struct), _hip.f64(ru, n2),
                _hip.f64(z[:n2], n2), _hip.f64(self.work, n2),
                _hip.stream()))
        return z

    def apply_fused(self, v, z):
        '''apply() with its first half -- the vmul, the copy and per coupling
        plane a product and an axpby -- in one launch (flow_mixed_upper_rhs,
        csrc/mixed_kernels.hip), then the unchanged ILU or Jacobi step: every
        entry of z has the bits apply() leaves there.  v overlapping z is a
        ValueError.'''
        n2 = self.n2
        upper_rhs(self.A, self.sinv, v, z[n2:], self.ru)
        if self.velocity == 'jacobi':
            ops.vmul(self.ru, self.dinv, z[:n2])
        else:
            _hip.check(_hip.lib().flow_ilu0_solve(
                ctypes.byref(self.ilu.struct), _hip.f64(self.ru, n2),
                _hip.f64(z[:n2], n2), _hip.f64(self.work, n2),
                _hip.stream()))
        return z

    def refresh(self, sdiag=None):
        '''The same object for new values in the planes of A (a Newton step:
        the buffers of A are held): Ilu0.refactor or a new inverse diagonal,
        and the signed Schur diagonal again unless sdiag gives one.'''
        if sdiag is None:
            sdiag = _signed_schur_diagonal(self.A, None)
        self.sinv = torch.reciprocal(sdiag)
        if self.velocity == 'ilu0':
            self.ilu.refactor(self.A.uu)
        else:
            self.dinv = self.A.uu.diag_inv()
        return self


def upper_rhs(A, sinv, r, zp, ru):
    '''z_p = r_p * sinv and ru = r_u - up z_p of the MixedMatrix A in one
    launch (flow_mixed_upper_rhs): r of 2 Nv + Np, sinv and zp of Np, ru of
    2 Nv doubles.  An output overlapping an input is a ValueError.'''
    n2, npr = A.W.size(), A.P.N
    _hip.check(_hip.lib().flow_mixed_upper_rhs(
        ctypes.byref(A.fused()), _hip.f64(sinv, npr, 'sinv'),
        _hip.f64(r, n2 + npr, 'r'), _hip.f64(zp, npr, 'z_p'),
        _hip.f64(ru, n2, 'ru'), _hip.stream()))
    return zp, ru


def _signed_schur_diagonal(A, pmask):
    '''diag(pp) - sum_s diag(pu[s] diag(uu_ss)^-1 up[s]) of the eliminated A,
    with its true sign: every entry of the plane pu[s] times its mirror entry
    of up[s] (_transpose_perm: the permutation symmetric_part uses), that
    plane applied to the inverse diagonal of uu's plane (s, s), summed.  A form
    written with -q*div(u) gives a negative, one with +q*div(u) a positive
    diagonal.  Rows with a zero and Dirichlet rows 1.'''
    nv, npr = A.W.N, A.P.N
    dinv = A.uu.diag_inv()
    if A.pp is not None:
        lay = A.pp.layout
        d = A.pp.vals[lay.dev('diag_idx').long()].contiguous()
    else:
        d = device.zeros(npr)
    tmp = device.empty(npr)
    for s in range(2):
        B, C = A.up[s], A.pu[s]
        if B is None or C is None:
            continue
        Rup, Rpu = B.layout, C.layout
        perm = _transpose_perm(Rpu, Rup).long()
        both = RectMatrix(Rpu)
        both.vals[:Rpu.nnz] = C.vals[:Rpu.nnz] * B.vals[perm]
        both.apply(dinv[s * nv:(s + 1) * nv], tmp)
        ops.axpby(-1.0, tmp, 1.0, d)
    one = torch.ones_like(d)
    d = torch.where(d != 0.0, d, one)
    if pmask is not None:
        d = torch.where(device.to_device(pmask) != 0, one, d)
    return d


def solver_route(symmetric, prm):
    '''Which loop solve() runs for a form that is symmetric (structurally, or
    by 'symmetric': True) or not: 'minres'; 'fgmres' with mixed_gmres(True)
    for a non-symmetric form, or where 'linear_solver' is 'gmres'; 'refuse'
    for a non-symmetric form with the switch off.'''
    from . import forms
    if forms.mixed_gmres.enabled and (
            not symmetric or prm.get('linear_solver') == 'gmres'):
        return 'fgmres'
    return 'minres' if symmetric else 'refuse'


def _validate_nullspace(ns, WP, bcs):
    '''nullspace.validate with the Dirichlet dofs of mixed_bcs: the checks of
    nullspace= that need no device.'''
    from . import nullspace
    held = mixed_bcs(bcs, WP)
    nullspace.validate(ns, WP, None if held is None else held[0])


def _deflated(ns, A, b, x, precondition, prm):
    '''What a linear solve with nullspace=ns runs before its loop: the |A z|
    check, b projected (its Z^T b and b . b left on the device: the slots of
    VectorSpaceBasis.project_rhs), the start vector x projected (None: a zero
    start), and the preconditioner wrapped so that every preconditioned
    vector is projected.  Returns (wrapped preconditioner, slots).'''
    from . import nullspace
    nullspace.check_null(ns, A, prm.get('nullspace_check'))
    slots = ns.project_rhs(b)
    if x is not None:
        ns.deflate(x)
    return nullspace.deflated_preconditioner(ns, precondition), slots


def _solve_fgmres(a, L, w, bcs, prm, form_compiler_parameters, nullspace=None):
    '''solve() for mixed_gmres(True): assemble_system (no symmetrisation of a
    non-symmetric form), BlockTriangularPreconditioner, fgmres.'''
    velocity = prm.get('preconditioner', 'ilu0')
    if velocity not in ('ilu0', 'jacobi'):
        raise ValueError("preconditioner %r under GMRES: 'ilu0' or 'jacobi'"
                         % (velocity,))
    ks = dict(prm.get('krylov_solver') or {})
    masks = {}
    if nullspace is not None:
        _validate_nullspace(nullspace, a.arguments()[0], bcs)
    A, b = assemble_system(a, L, bcs, form_compiler_parameters, masks)
    if A.uu is None:
        raise ValueError('the form has no velocity-velocity block')
    if prm.get('preconditioner_form') is not None:
        sdiag = _form_diagonal(prm['preconditioner_form'], bcs,
                               form_compiler_parameters, signed=True)
    else:
        sdiag = _signed_schur_diagonal(A, masks['p'])
    M = BlockTriangularPreconditioner(A, velocity, sdiag)
    precondition, slots = M.apply, None
    if nullspace is not None:
        # (the true residual of fgmres is then taken against the projected b)
        precondition, slots = _deflated(nullspace, A, b.data, w.data, M.apply,
                                        prm)
    # (the one-launch product: bit-equal to A.apply and faster, README)
    its, res = fgmres(A.apply_fused, precondition, b.data, w.data,
                      ks.get('relative_tolerance', 1.0e-12),
                      ks.get('absolute_tolerance', 0.0),
                      int(ks.get('maximum_iterations', 1000)),
                      int(ks.get('restart', 30)))
    info = ops.SolveInfo(its, res, 'fgmres+' + velocity)
    if slots is not None:
        info.rhs_defect = nullspace.defect(slots)
    return info


def solve(a, L, w, bcs=None, solver_parameters=None,
          form_compiler_parameters=None, nullspace=None):
    '''solve(a == L, w, bcs) with w = Function(WP): assemble_system, then
    preconditioned MINRES from w's values into w.  MINRES takes a symmetric
    form -- structurally (forms.is_symmetric_form: over all its parts) or by
    solver_parameters['symmetric'] = True.  Any other form is a
    NotImplementedError unless forms.mixed_gmres(True) is on (assemble_system
    and to_scipy() work for it either way); with that switch it goes to
    assemble_system without symmetrisation, BlockTriangularPreconditioner and
    fgmres over apply_fused, and 'linear_solver': 'gmres' sends a symmetric
    form there too.  There: 'preconditioner' 'ilu0' (default) | 'jacobi'
    ('two_level' is a ValueError); 'preconditioner_form', whose pp block's
    SIGNED lumped rows as written precondition the pressure (-p*q*dx, or
    -(1/nu)*p*q*dx for Oseen, for the reference's sign convention; default:
    _signed_schur_diagonal); 'krylov_solver' also takes 'restart' (30), and
    the tolerances are on the true residual |b - A x|_2; the method reported
    is 'fgmres+ilu0' or 'fgmres+jacobi'; a matrix without a uu block is a
    ValueError.
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
    nothing pinned) takes nullspace=fem.constant_nullspace(WP) (fem/
    nullspace.py; the checks and rhs_defect: ops.solve's docstring): b and
    the start vector are projected once, and every preconditioned vector of
    the loop -- z_new of minres, the output of precondition in fgmres -- by a
    wrapped preconditioner; minres and fgmres themselves are unchanged, and
    fgmres tests the true residual against the projected b.  The left and the
    right nullspace must coincide.  Returns an ops.SolveInfo; raises
    _hip.NotConverged.'''
    from . import forms
    WP = a.arguments()[0]
    if not isinstance(w, Function) or not forms.is_mixed_space(
            w.function_space()) or not w.function_space().same_as(WP):
        raise ValueError('solve writes into a Function of the space of the '
                         'trial function')
    prm = dict(solver_parameters or {})
    symmetric = prm.get('symmetric') is True or forms.is_symmetric_form(a)
    route = solver_route(symmetric, prm)
    if route == 'refuse':
        raise NotImplementedError(
            'solve of a non-symmetric form on a mixed space: MINRES needs a '
            'symmetric form; flexible GMRES with a block preconditioner '
            'takes it once fem.mixed_gmres(True) is on; assemble_system(a, '
            'L, bcs) and to_scipy() work for it either way')
    if route == 'fgmres':
        return _solve_fgmres(a, L, w, bcs, prm, form_compiler_parameters,
                             nullspace)
    ks = dict(prm.get('krylov_solver') or {})
    masks = {}
    if nullspace is not None:
        _validate_nullspace(nullspace, WP, bcs)
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
    precondition, slots = M.apply, None
    if nullspace is not None:
        precondition, slots = _deflated(nullspace, A, b.data, w.data, M.apply,
                                        prm)
    its, res = minres(A.apply, precondition, b.data, w.data,
                      ks.get('relative_tolerance', 1.0e-12),
                      ks.get('absolute_tolerance', 0.0),
                      int(ks.get('maximum_iterations', 1000)))
    info = ops.SolveInfo(its, res, 'minres')
    if slots is not None:
        info.rhs_defect = nullspace.defect(slots)
    return info


# -- Newton's method on WP: solve(F == 0, w, bcs) -----------------------------------
BLOCK_NAMES = ('uu', 'pp', 'up0', 'up1', 'pu0', 'pu1')

# The rule of adoption (README): the Newton path runs
# BlockTriangularPreconditioner.apply_fused where its measured median is not
# above apply's (tools/mixed_newton_lab.py), else apply.
NEWTON_FUSED_PRECONDITIONER = True


def _table_blocks(table):
    '''{block name: [scalar tables]} of a rank-2 MixedTable: the four tables
    of the velocity corner under 'uu'.'''
    out = {k: [] for k in BLOCK_NAMES}
    for r in range(2):
        for s in range(2):
            if table[r][s] is not None:
                out['uu'].append(table[r][s])
        if table[r][2] is not None:
            out['up%d' % r].append(table[r][2])
        if table[2][r] is not None:
            out['pu%d' % r].append(table[2][r])
    if table[2][2] is not None:
        out['pp'].append(table[2][2])
    return out


def _reads(tree, WP, w):
    '''forms.depends_on(tree, w); w None: whether the tree reads a view of
    any Function of the space WP.'''
    from . import forms
    if w is not None:
        return forms.depends_on(tree, w)
    if tree[0] == 'field':
        own = getattr(tree[1], 'mixed_owner', None)
        return own is not None and own[0].function_space().same_as(WP)
    return tree[0] in forms.NONLEAF and any(
        _reads(c, WP, None) for c in tree[1:] if isinstance(c, tuple))


def block_dependence(J, WP, w=None):
    '''{block name: whether a part of the rank-2 mixed form J has a term of
    that block that reads w} over the blocks J has a term for.'''
    from . import forms
    out = {}
    for _, part in J.terms():
        _, table = part.argument_table()
        if not isinstance(table, forms.MixedTable):
            raise NotImplementedError(forms._MIXED_MISMATCH)
        for name, tabs in _table_blocks(table).items():
            for tab in tabs:
                reads = any(c is not None and _reads(c, WP, w)
                            for row in tab for c in row)
                out[name] = out.get(name, False) or reads
    return out


class MixedNewtonAssembler(object):
    '''(J, F) of Newton's method on the Taylor-Hood space WP at the current
    values of the fields: a MixedMatrix and a vector of 2 Nv + Np whose
    buffers live as long as the object.  Every block of J has the bits of
    assemble(J) and every component of F those of assemble(F): the launches
    are assemble_form's -- the velocity corner through ops._block_part, pp
    through ops._scalar_part, the coupling planes through _rect_part --, their
    results copied into the held planes.
    `frozen`: the blocks of J (MixedMatrix.blocks() naming) none of whose
    parts reads w (forms.depends_on; w None: a view of any Function of WP) --
    for Navier-Stokes up0, up1, pu0, pu1 and any pp.  A frozen block is
    assembled by the first assemble() and not again; system() applies the
    boundary conditions to it once.  `route` is 'by_parts': every part is
    assembled on its own; there is no fused element kernel here.'''
    route = 'by_parts'
    fused = False

    def __init__(self, J, F, WP, form_compiler_parameters=None, w=None):
        from . import forms
        if not forms.vector_arguments.enabled:
            raise NotImplementedError(
                'forms on a mixed space need vector_arguments(True) as well')
        self.space = WP
        self.J, self.F = J, F
        self.params = form_compiler_parameters
        for form in (J, F):
            for _, part in form.terms():
                ops._check_part_mesh(part, WP.mesh())
        reads = block_dependence(J, WP, w)
        self.frozen = tuple(k for k in BLOCK_NAMES
                            if k in reads and not reads[k])
        self._live = tuple(k for k in BLOCK_NAMES if reads.get(k))
        self.A = None
        self.b = device.empty(WP.size())
        self._system = None

    @staticmethod
    def _block(A, name):
        return {'uu': A.uu, 'pp': A.pp}[name] if len(name) == 2 else \
            (A.up if name[:2] == 'up' else A.pu)[int(name[2])]

    def assemble(self):
        '''(MixedMatrix, device vector): the held J and F, without boundary
        conditions.'''
        if self.A is None:
            # (the first call: all blocks; the result's planes are the held
            # ones from here on)
            self.A = assemble_form(self.J, 2, self.params)
        elif self._live:
            fresh = assemble_form(self.J, 2, self.params, only=self._live)
            for name in self._live:
                _hip.copy(self._block(self.A, name).vals,
                          self._block(fresh, name).vals)
        _hip.copy(self.b, assemble_form(self.F, 1, self.params).data)
        return self.A, self.b

    def system(self, um, pm):
        '''The held J with the conditions of the device masks um (2 Nv bytes)
        and pm (Np bytes) applied homogeneously, as assemble_system applies
        them: symmetric_bc_blocks on uu, symmetric_bc_matrix on pp (absent
        and a pressure condition: unit diagonal on its rows),
        flow_bc_rect_mask on the coupling planes.  Into held planes of its
        own; a frozen block only the first time.  After assemble().'''
        A = self.A
        W, P = A.W, A.P
        nv = W.N
        first = self._system is None
        if first:
            uu = None if A.uu is None else ops.Matrix(W.layout, 2)
            pp = None
            if A.pp is not None or bool(pm.any()):
                pp = ops.Matrix(P.layout, 0)
            self._system = MixedMatrix(
                self.space, uu, pp,
                [None if B is None else RectMatrix(B.layout) for B in A.up],
                [None if B is None else RectMatrix(B.layout) for B in A.pu])
            self._pp_zero = None if A.pp is not None or pp is None \
                else ops.Matrix(P.layout, 0)
        S = self._system
        todo = lambda k: first or k in self._live   # noqa: E731
        if A.uu is not None and todo('uu'):
            ops.symmetric_bc_blocks(A.uu, um, S.uu)
        if A.pp is not None and todo('pp'):
            ops.symmetric_bc_matrix(A.pp, pm, S.pp)
        elif first and S.pp is not None and A.pp is None:
            ops.symmetric_bc_matrix(self._pp_zero, pm, S.pp)
        ums = [um[r * nv:(r + 1) * nv] for r in range(2)]
        for c in range(2):
            if A.up[c] is not None and todo('up%d' % c):
                _hip.copy(S.up[c].vals, A.up[c].vals)
                _rect_mask(S.up[c], ums[c], pm)
            if A.pu[c] is not None and todo('pu%d' % c):
                _hip.copy(S.pu[c].vals, A.pu[c].vals)
                _rect_mask(S.pu[c], pm, ums[c])
        return S


def newton_solve(F, w, bcs=None, J=None, solver_parameters=None,
                 form_compiler_parameters=None, nullspace=None):
    '''solve(F == 0, w, bcs, J) with w a Function of the Taylor-Hood space WP
    (forms.mixed_derivatives(True)): ops.newton_solve's loop -- its order,
    stopping rule, 'newton_solver' keys and defaults (ops.newton_parameters),
    'report' and 'error_on_nonconvergence' -- over MixedNewtonAssembler.
    w[dof] = g first (mixed_bcs); per iteration (J, F) at w, the conditions
    applied homogeneously (MixedNewtonAssembler.system, F[dof] = 0), r =
    |F|_2, stop where r < absolute_tolerance or r / r0 < relative_tolerance,
    else J delta = F from a zero start by fgmres over apply_fused with
    BlockTriangularPreconditioner -- the ILU(0) factors refactored and the
    signed Schur diagonal recomputed every step (unless 'preconditioner_form'
    gives one) -- and w -= relaxation_parameter * delta.
    'newton_solver' also takes 'preconditioner' ('ilu0' | 'jacobi';
    'two_level' is the ValueError of the linear solve) and
    'preconditioner_form', and its 'krylov_solver' 'restart', with the
    meanings of solve(a == L) under mixed_gmres.  Needs mixed_gmres(True).  A
    singular pressure takes nullspace=fem.constant_nullspace(WP): every
    step's J delta = F goes through the deflated solve of solve(a == L)
    (solver_parameters['nullspace_check'] as there), so delta has no
    component along the basis and w keeps the pressure mean it started with;
    the info's rhs_defect is the largest |Z^T F| / |F| over the steps.
    Returns an ops.NewtonInfo with
    `frozen` (MixedNewtonAssembler.frozen), route 'by_parts' and method
    'fgmres+ilu0' | 'fgmres+jacobi'.  Not on strips.'''
    from . import forms
    from ..message import info as say
    prm = dict(solver_parameters or {})
    ns_prm = {}
    if nullspace is not None and 'nullspace_check' in prm:
        ns_prm['nullspace_check'] = prm.pop('nullspace_check')
    given = dict(prm.get('newton_solver') or {})
    velocity = given.pop('preconditioner', 'ilu0')
    prec_form = given.pop('preconditioner_form', None)
    if 'newton_solver' in prm:
        prm['newton_solver'] = given
    ns, _ = ops.newton_parameters(prm)
    if velocity not in ('ilu0', 'jacobi'):
        raise ValueError("preconditioner %r under GMRES: 'ilu0' or 'jacobi'"
                         % (velocity,))
    if not isinstance(F, forms.Form) or F.rank != 1:
        raise ValueError('solve(F == 0, w): F must be a form of rank 1, '
                         'linear in the test functions')
    WP = w.function_space()
    V = F.arguments()[0]
    if not forms.is_mixed_space(V) or not V.same_as(WP) \
            or not getattr(w, '_mixed', False):
        raise ValueError('solve writes into a Function of the space of the '
                         'test functions')
    for _, part in F.terms():
        if part.integral_type == 'interior_facet':
            raise NotImplementedError(
                'solve(F == 0) on a mixed space: dS parts are not supported '
                '(test functions under dS)')
    if not any(forms.depends_on(p.integrand.comps, w) for _, p in F.terms()):
        raise ValueError('solve(F == 0, w): the form does not depend on w')
    if J is None:
        J = forms.derivative(F, w)
    elif not isinstance(J, forms.Form) or J.rank != 2 \
            or not all(forms.is_mixed_space(S) and S.same_as(WP)
                       for S in J.arguments().values()):
        raise ValueError('J must be a bilinear form (rank 2) on the space of '
                         'w')
    if not forms.mixed_gmres.enabled:
        raise NotImplementedError(
            'solve(F == 0) on a mixed space: the Jacobian is not symmetric and '
            'its linear solves are flexible GMRES with a block preconditioner, '
            'which fem.mixed_gmres(True) switches on')
    if nullspace is not None:
        _validate_nullspace(nullspace, WP, bcs)
    asm = MixedNewtonAssembler(J, F, WP, form_compiler_parameters, w)
    ks = ns['krylov_solver']
    held = mixed_bcs(bcs, WP)
    W, P = WP.taylor_hood()
    if held is None:
        dofs = None
        um = device.to_device(numpy.zeros(W.size(), dtype=numpy.uint8))
        pm = device.to_device(numpy.zeros(P.size(), dtype=numpy.uint8))
        pmask = None
    else:
        dofs, vals = device.to_device(held[0]), device.to_device(held[1])
        um, pm = device.to_device(held[2]), device.to_device(held[3])
        pmask = held[3]
        ops._set_values(dofs, vals, w.data)
        zero = device.zeros(dofs.numel())
    sform = None
    if prec_form is not None:
        sform = _form_diagonal(prec_form, bcs, form_compiler_parameters,
                               signed=True)
    delta = device.empty(WP.size())
    M = None
    out = ops.NewtonInfo(False, 'fgmres+' + velocity, asm.route)
    out.frozen = asm.frozen
    rtol, atol = ns['relative_tolerance'], ns['absolute_tolerance']
    maxit = int(ns['maximum_iterations'])
    r0 = None
    while True:
        asm.assemble()
        A = asm.system(um, pm)
        b = asm.b
        if dofs is not None:
            ops._set_values(dofs, zero, b)
        r = ops.vector_norm(b)
        r0 = r if r0 is None else r0
        out.residuals.append(r)
        rel = r / r0 if r0 > 0.0 else 0.0
        if ns['report']:
            say('Newton iteration %d: r (abs) = %.3e (tol = %.3e) r (rel) = '
                '%.3e (tol = %.3e)' % (out.iterations, r, atol, rel, rtol))
        if r < atol or rel < rtol:
            out.converged = True
            break
        if out.iterations >= maxit:
            break
        if A.uu is None:
            raise ValueError('the form has no velocity-velocity block')
        sdiag = sform if sform is not None \
            else _signed_schur_diagonal(A, pmask)
        if M is None:
            M = BlockTriangularPreconditioner(A, velocity, sdiag)
        else:
            M.refresh(sdiag)
        _hip.fill(delta, 0.0)
        precondition = M.apply_fused if NEWTON_FUSED_PRECONDITIONER \
            else M.apply
        slots = None
        if nullspace is not None:
            precondition, slots = _deflated(nullspace, A, b, None,
                                            precondition, ns_prm)
            # (the |A z| check: on the first Jacobian only)
            ns_prm = {'nullspace_check': False}
        its, _ = fgmres(
            A.apply_fused, precondition,
            b, delta, ks.get('relative_tolerance', 1.0e-12),
            ks.get('absolute_tolerance', 0.0),
            int(ks.get('maximum_iterations', 1000)),
            int(ks.get('restart', 30)))
        if slots is not None:
            out.rhs_defect = max(out.rhs_defect or 0.0,
                                 nullspace.defect(slots))
        out.linear_iterations.append(its)
        ops.axpby(-float(ns['relaxation_parameter']), delta, 1.0, w.data)
        out.iterations += 1
    if not out.converged and ns['error_on_nonconvergence']:
        raise _hip.NotConverged(
            'Newton solver did not converge: %d iterations, |F| = %.3e '
            '(absolute tolerance %.3e), |F| / |F0| = %.3e (relative '
            'tolerance %.3e)' % (out.iterations, r, atol, rel, rtol))
    return out
