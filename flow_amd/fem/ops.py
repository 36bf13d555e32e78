# -*- coding: utf-8 -*-
'''
Host-side operations that run on the HIP path: matrices over a space's CSR
pattern, Krylov solves, norms, and the callers' utilities `project`,
`interpolate`, `errornorm`, `norm` (tests/test_navier_stokes.py:296-308, 333;
tests/test_karman_vortex_street.py:262-268; tests/test_boussinesq.py:85),
`assemble` / `assemble_system` / `solve` of forms (flow_amd/fem/forms.py):
`solve(a == L, u, bcs)` a Krylov solve, `solve(F == 0, u, bcs, J)` Newton's
method with the Jacobian and the residual assembled in one pass
(newton_solve, NewtonAssembler, flow_form_newton; on vector spaces
flow_form_block_newton).

Everything numerical is a call into libflow_hip.so (flow_amd/_hip.py); torch
only owns the HBM buffers.
'''
import collections
import ctypes
import functools
import itertools
import numbers

import numpy
import torch

from . import reference
from .function import (
    Function, Expression, Constant, as_cell_coefficient, cell_lattice_points,
    )
from .selection import (        # noqa: F401  (ops' names for them stay)
    InteriorFacetLists, facet_lists, interior_facet_lists, cell_lists,
    facet_map_host, facet_map, cell_map_host, cell_map, is_cell_subdomain,
    _facet_selection, _cell_selection, _check_cell_markers,
    )
from .space import mesh_geometry_dev
from .. import _hip
from .. import device


# -- C structs ----------------------------------------------------------------
def mesh_struct(mesh):
    if 'mesh_struct' not in mesh._cache:
        xy = mesh_geometry_dev(mesh)
        s = _hip.MeshS(mesh.num_cells(), _hip.f64(xy, 6 * mesh.num_cells(), 'xy'))
        mesh._cache['mesh_struct'] = (s, xy)
    return mesh._cache['mesh_struct'][0]


def space_struct(layout):
    if 'struct' not in layout._dev:
        nc = layout.mesh.num_cells()
        cd = layout.dev('cell_dofs')
        s = _hip.SpaceS(
            layout.degree, layout.N, layout.nnz,
            _hip.i32(cd, layout.nloc * nc, 'cell_dofs'),
            _hip.i32(layout.dev('cptr'), layout.nnz + 1, 'cptr'),
            _hip.i32(layout.dev('csrc'), layout.nloc**2 * nc, 'csrc'),
            _hip.i32(layout.dev('vptr'), layout.N + 1, 'vptr'),
            _hip.i32(layout.dev('vsrc'), layout.nloc * nc, 'vsrc'),
            )
        layout._dev['struct'] = s
    return layout._dev['struct']


_G_CACHE = {}


def coef_struct(coef, mesh, test_degree):
    '''flow_coef of a CellCoefficient for test functions of `test_degree`.
    Returns (struct, keepalive).'''
    key = (coef.k, test_degree, str(device.get()))
    if key not in _G_CACHE:
        _G_CACHE[key] = device.to_device(
            reference.source_matrix(coef.k, test_degree)
            )
    G = _G_CACHE[key]
    nce = mesh.num_cells() if coef.cell_stride else 1
    s = _hip.CoefS(
        coef.nl, coef.cell_stride,
        _hip.f64(coef.values, coef.dim * coef.nl * nce, 'coefficient values'),
        _hip.f64(G, coef.nl * reference.nloc(test_degree), 'G'),
        )
    return s, (coef.values, G)


def scratch(mesh, ndoubles):
    '''Per-mesh scratch buffer for the cell kernels (grown on demand).'''
    buf = mesh._cache.get('scratch')
    if buf is None or buf.numel() < ndoubles:
        mesh._cache['scratch'] = None
        buf = device.empty(ndoubles)
        mesh._cache['scratch'] = buf
    if device._POISON:      # debugging aid: stale scratch reads become NaNs
        _hip.fill(buf, float('nan'))
    return buf


_WORK = {}


def work(ndoubles):
    key = str(device.get())
    buf = _WORK.get(key)
    if buf is None or buf.numel() < ndoubles:
        _WORK[key] = None
        buf = device.empty(ndoubles)
        _WORK[key] = buf
    return buf


# -- matrices -----------------------------------------------------------------
def plane_stride(layout):
    '''Distance between value planes: nnz rounded up to even, so that every
    plane is 16-byte aligned and readable one entry past nnz (the SpMV loads
    value pairs; include/flow_hip.h, flow_operator).'''
    return layout.nnz + (layout.nnz & 1)


def value_plane(layout):
    return device.zeros(plane_stride(layout))


class Matrix(object):
    '''Value planes over the CSR pattern of a scalar layout.
    kind 0: scalar (1 plane), 1: block-diagonal (2 planes), 2: 2x2 (4 planes),
    4: one plane for both components of a vector field with identity rows
    where `rowmask` (uint8, 2N) is 0 (include/flow_hip.h, flow_operator);
    `vals` is one tensor of nplanes*stride doubles, stride = plane_stride().'''
    NPLANES = {0: 1, 1: 2, 2: 4, 4: 1}

    def __init__(self, layout, kind, vals=None, rowmask=None):
        self.layout = layout
        self.kind = kind
        assert (rowmask is not None) == (kind == 4)
        if rowmask is not None:
            assert rowmask.dtype == torch.uint8 and \
                rowmask.numel() == 2 * layout.N
        self.rowmask = rowmask
        self.nplanes = self.NPLANES[kind]
        nnz = layout.nnz
        self.stride = plane_stride(layout)
        if vals is None:
            vals = device.zeros(self.nplanes * self.stride)
        elif vals.numel() == self.nplanes * nnz and self.stride != nnz:
            # compact planes -> aligned planes
            packed = device.zeros(self.nplanes * self.stride)
            for p in range(self.nplanes):
                packed[p * self.stride:p * self.stride + nnz] = \
                    vals[p * nnz:(p + 1) * nnz]
            vals = packed
        assert vals.numel() == self.nplanes * self.stride
        assert vals.data_ptr() % 16 == 0
        self.vals = vals
        self._op = None
        return

    @property
    def size(self):
        return self.layout.N * (1 if self.kind == 0 else 2)

    def plane(self, p):
        return self.vals[p * self.stride:p * self.stride + self.layout.nnz]

    def operator(self):
        if self._op is None:
            lay = self.layout
            op = _hip.Operator()
            op.kind = self.kind
            op.n = lay.N
            op.nnz = lay.nnz
            rb = lay.dev('rowblocks2' if self.kind in (2, 4) else 'rowblocks')
            op.nblocks = rb.numel() - 1
            op.rowptr = _hip.i32(lay.dev('rowptr'), lay.N + 1, 'rowptr')
            op.cols = _hip.i32(lay.dev('cols'), lay.nnz, 'cols')
            op.rowblocks = _hip.i32(rb, None, 'rowblocks')
            base = _hip.f64(self.vals, self.nplanes * self.stride, 'vals').value
            for p in range(self.nplanes):
                op.vals[p] = base + 8 * p * self.stride
            if self.rowmask is not None:
                op.rowmask = _hip.u8(self.rowmask, 2 * lay.N, 'rowmask').value
            self._op = op
        return self._op

    def apply(self, x, y):
        lib = _hip.lib()
        assert x.data_ptr() != y.data_ptr()
        _hip.check(lib.flow_operator_apply(
            ctypes.byref(self.operator()), _hip.f64(x, self.size, 'x'),
            _hip.f64(y, self.size, 'y'), _hip.stream()
            ))
        return y

    def apply_block(self, X, ldx, m, Y, ldy, chunk=0):
        '''Y[:, j] = A X[:, j] for the first m columns of the column stores X
        and Y (tensors, column strides ldx and ldy: >= self.size and even, the
        stores 16-byte aligned, Y not overlapping X): one launch that reads
        the matrix once; every column has the bits of apply() on that column
        (flow_operator_apply_block).  Scalar matrices (kind 0: columns of N
        entries) and 2x2-block matrices (kind 2: columns of 2N entries,
        component-blocked, all four value planes read once); other kinds are
        a ValueError.  chunk: columns a workgroup takes at a time (2, 4, and
        for kind 0 also 8; 0: the library's choice).'''
        lib = _hip.lib()
        if self.kind not in (0, 2):
            raise ValueError('apply_block: a scalar or a 2x2-block matrix '
                             '(kind 0 or 2), not kind %d' % self.kind)
        m = int(m)
        if m == 0:
            return Y
        n = self.size
        _hip.check(lib.flow_operator_apply_block_chunk(
            ctypes.byref(self.operator()), m,
            _hip.f64(X, (m - 1) * ldx + n, 'X'), ldx,
            _hip.f64(Y, (m - 1) * ldy + n, 'Y'), ldy, int(chunk),
            _hip.stream()))
        return Y

    def diag_inv(self):
        lib = _hip.lib()
        out = device.empty(self.size)
        _hip.check(lib.flow_operator_diag_inv(
            ctypes.byref(self.operator()),
            _hip.i32(self.layout.dev('diag_idx'), self.layout.N, 'diag_idx'),
            _hip.f64(out), _hip.stream()
            ))
        return out

    def __mul__(self, x):
        '''A * x for a Vector or a Function: a new Vector (one apply).  Not
        on strips, where a rank holds its own rows only.'''
        from .function import Vector
        _no_strips('Matrix * vector')
        data = x.data if isinstance(x, (Vector, Function)) else None
        if data is None:
            return NotImplemented
        if data.numel() != self.size:
            raise ValueError('matrix of size %d times a vector of %d entries'
                             % (self.size, data.numel()))
        return Vector(self.apply(data, device.empty(self.size)))

    __matmul__ = __mul__

    def to_scipy(self):
        '''Host copy as a scipy.sparse CSR matrix: the way to inspect an
        assembled matrix (entries, symmetry, a direct solve in a test).  Not
        for hot paths: it copies every value plane to the host.'''
        import scipy.sparse as sp
        lay = self.layout
        rp = lay.pattern('rowptr')
        cols = lay.pattern('cols')
        v = device.to_host(self.vals).numpy()
        nnz = lay.nnz
        st = self.stride
        P = [sp.csr_matrix((v[p * st:p * st + nnz], cols, rp),
                           shape=(lay.N, lay.N)) for p in range(self.nplanes)]
        if self.kind == 0:
            return P[0]
        if self.kind == 4:
            m = device.to_host(self.rowmask).numpy().astype(float)
            blocks = [
                sp.diags(m[c * lay.N:(c + 1) * lay.N]).dot(P[0])
                + sp.diags(1.0 - m[c * lay.N:(c + 1) * lay.N])
                for c in range(2)
                ]
            return sp.block_diag(blocks, format='csr')
        if self.kind == 1:
            return sp.block_diag(P, format='csr')
        return sp.bmat([[P[0], P[1]], [P[2], P[3]]], format='csr')


class MomentumJacobian(object):
    '''Matrix-free Jacobian of the momentum residual at `ui` (flow_operator
    kind 3, include/flow_hip.h `flow_momentum_jvp`): `derivative(F1, ui)` of the
    reference (pressure_correction.py:202) applied cell by cell instead of
    assembled.  Quacks like a Matrix for krylov_solve ('bicgstab').'''
    kind = 3

    def __init__(self, W, bfmask, ui, prm, bc_dofs, mesh_s=None, space_s=None):
        '''mesh_s / space_s: a rank's views of the mesh and space structs
        (cell and row ranges: flow_amd/parallel.py); default: everything.'''
        mesh = W.mesh()
        self.layout = W.layout
        self.size = W.size()
        n2 = self.size
        nc = mesh.num_cells()
        if mesh_s is None:
            mesh_s = mesh_struct(mesh)
        if space_s is None:
            space_s = space_struct(W.layout)
        self._keep = (bfmask, ui, bc_dofs,
                      device.empty(2 * W.layout.nloc * nc), mesh_s, space_s)
        self.struct = _hip.MomentumJvp(
            ctypes.pointer(mesh_s),
            ctypes.pointer(space_s),
            _hip.i32(bfmask, nc, 'bfmask'), _hip.f64(ui, n2, 'ui'), prm,
            _hip.f64(self._keep[3]), int(bc_dofs.numel()),
            _hip.i32(bc_dofs) if bc_dofs.numel() else None,
            self._bc_mask(bc_dofs),
            )
        op = _hip.Operator()
        op.kind = 3
        op.n = W.layout.N
        op.matfree = ctypes.cast(ctypes.pointer(self.struct), ctypes.c_void_p)
        self._op = op

    def operator(self):
        return self._op

    def _bc_mask(self, bc_dofs):
        '''Byte mask of the Dirichlet dofs (2n, component-blocked): with it the
        gather of an application writes the identity rows itself.  Built once
        per dof set (the caller hands in the same tensor while the conditions
        are unchanged).'''
        if not bc_dofs.numel():
            return None
        held = getattr(self, '_mask', None)
        # (the same tensor, not rewritten in place since: identity alone would
        # keep a stale mask after an in-place update of the dof list)
        stamp = (bc_dofs.data_ptr(), bc_dofs.numel(), bc_dofs._version)
        if held is None or held[0] is not bc_dofs or held[2] != stamp:
            mask = torch.zeros(self.size, dtype=torch.uint8,
                               device=bc_dofs.device)
            mask[bc_dofs.long()] = 1
            device.synchronize()
            self._mask = held = (bc_dofs, mask, stamp)
        return _hip.u8(held[1], self.size, 'bc_mask')

    def rebind(self, bfmask, ui, prm, bc_dofs):
        '''Point the operator at another linearisation state (a time loop
        builds one per Newton iteration: the 0.2 GB scratch buffer and the
        structs stay).'''
        nc = self.layout.mesh.num_cells()
        self._keep = (bfmask, ui, bc_dofs) + self._keep[3:]
        s = self.struct
        s.bfmask = _hip.i32(bfmask, nc, 'bfmask')
        s.ui = _hip.f64(ui, self.size, 'ui')
        s.prm = prm
        s.nbc = int(bc_dofs.numel())
        s.bc_dofs = _hip.i32(bc_dofs) if bc_dofs.numel() else None
        s.bc_mask = self._bc_mask(bc_dofs)
        return self

    @classmethod
    def cached(cls, W, bfmask, ui, prm, bc_dofs, mesh_s=None, space_s=None):
        '''The operator of W's layout, created on first use and re-pointed
        afterwards.'''
        key = ('jvp_operator', id(mesh_s), id(space_s))
        held = W.layout._dev.get(key)
        if held is None:
            held = cls(W, bfmask, ui, prm, bc_dofs, mesh_s, space_s)
            W.layout._dev[key] = held
            return held
        return held.rebind(bfmask, ui, prm, bc_dofs)

    def apply(self, x, y):
        lib = _hip.lib()
        assert x.data_ptr() != y.data_ptr()
        _hip.check(lib.flow_momentum_jvp_apply(
            ctypes.byref(self.struct), _hip.f64(x, self.size, 'x'),
            _hip.f64(y, self.size, 'y'), _hip.stream()
            ))
        return y


STIFFNESS, MASS, LUMPED_MASS = 0, 1, 2


def assemble_scalar_matrix(layout, kind):
    '''Step-invariant scalar matrices, cached per layout (K1, K3).'''
    key = ('matrix', kind)
    if key not in layout._dev:
        lib = _hip.lib()
        mesh = layout.mesh
        A = Matrix(layout, 0)
        buf = scratch(mesh, layout.nloc**2 * mesh.num_cells())
        _hip.check(lib.flow_assemble_scalar_matrix(
            kind, ctypes.byref(mesh_struct(mesh)),
            ctypes.byref(space_struct(layout)), _hip.f64(buf),
            _hip.f64(A.vals), _hip.stream()
            ))
        layout._dev[key] = A
    return layout._dev[key]


def assemble_mass(V):
    return assemble_scalar_matrix(V.layout, MASS)


def assemble_stiffness(V):
    return assemble_scalar_matrix(V.layout, STIFFNESS)


def symmetric_bc_matrix(A, isbc, out=None):
    '''assemble_system-style symmetric elimination of one scalar plane
    (out: a Matrix of the same layout to write into).'''
    lib = _hip.lib()
    lay = A.layout
    if out is None:
        out = Matrix(lay, 0)
    _hip.check(lib.flow_bc_symmetric_matrix(
        lay.N, _hip.i32(lay.dev('rowptr')), _hip.i32(lay.dev('cols')),
        _hip.f64(A.vals, lay.nnz), _hip.u8(isbc, lay.N, 'isbc'),
        _hip.f64(out.vals, lay.nnz), _hip.stream()
        ))
    return out


def symmetric_bc_blocks(A, isbc, out=None):
    '''symmetric_bc_matrix for the four planes of a kind-2 Matrix in one
    launch; isbc: 2N bytes in operator numbering.'''
    lib = _hip.lib()
    lay = A.layout
    assert A.kind == 2
    if out is None:
        out = Matrix(lay, 2)
    _hip.check(lib.flow_bc_symmetric_blocks(
        lay.N, lay.nnz, _hip.i32(lay.dev('rowptr')), _hip.i32(lay.dev('cols')),
        _hip.f64(A.vals, 4 * A.stride), A.stride,
        _hip.u8(isbc, 2 * lay.N, 'isbc'), _hip.f64(out.vals, 4 * out.stride),
        out.stride, _hip.stream()
        ))
    return out


class CoarseSpace(object):
    '''Piecewise-constant aggregate coarse space of a scalar SPD operator for
    the two-level additive preconditioner of flow_cg_solve (include/flow_hip.h,
    `flow_coarse`): dofs are binned into square patches of `s` mesh widths,
    Dirichlet dofs are left out, Ac = P^T A P is inverted densely on the host
    once per (operator, BC set).  `singular`: pure Neumann operator (constants
    in the kernel) -> pseudo-inverse via the rank-one shift.  Setup only; the
    per-iteration work runs in the HIP kernels.'''

    def __init__(self, A, isbc=None, singular=False, target_nc=4096):
        import scipy.sparse as sp
        lay = A.layout
        n = lay.N
        assert A.kind == 0
        isbc = numpy.zeros(n, dtype=bool) if isbc is None else \
            numpy.asarray(isbc, dtype=bool)
        x = lay.dof_coords
        h = numpy.sqrt(2.0 * lay.mesh.cell_areas().mean())
        nfree = int(n - isbc.sum())
        s = max(2.0, numpy.sqrt(max(nfree, 1) / float(target_nc)))
        while True:
            ix = numpy.floor((x[:, 0] - x[:, 0].min()) / (s * h) + 1e-9)
            iy = numpy.floor((x[:, 1] - x[:, 1].min()) / (s * h) + 1e-9)
            key = (ix * 2000003 + iy).astype(numpy.int64)
            key[isbc] = -1
            ukey, agg = numpy.unique(key, return_inverse=True)
            if len(ukey) and ukey[0] == -1:
                agg = agg - 1          # excluded dofs -> -1
                nc = len(ukey) - 1
            else:
                nc = len(ukey)
            if nc <= 1.25 * target_nc or s > 1.0e6:
                break
            s *= 1.1
        assert nc >= 1
        self.s = s
        self.nc = nc
        self.n = n
        free = numpy.nonzero(agg >= 0)[0]
        Pm = sp.csr_matrix(
            (numpy.ones(len(free)), (free, agg[free])), shape=(n, nc)
            )
        Ah = A.to_scipy()
        Ac = (Pm.T.dot(Ah).dot(Pm)).toarray()
        if singular:
            e = numpy.ones(nc)
            beta = numpy.trace(Ac) / nc
            Ainv = numpy.linalg.inv(Ac + beta * numpy.outer(e, e) / nc) \
                - numpy.outer(e, e) / (beta * nc)
        else:
            Ainv = numpy.linalg.inv(Ac)
        Ainv = 0.5 * (Ainv + Ainv.T)
        order = numpy.argsort(agg[free], kind='stable')
        agg_dofs = free[order].astype(numpy.int32)
        agg_ptr = numpy.zeros(nc + 1, dtype=numpy.int64)
        numpy.cumsum(numpy.bincount(agg[free], minlength=nc), out=agg_ptr[1:])
        self.agg_of_host = agg.astype(numpy.int32)
        # fp32 storage, rows padded to a multiple of 4 floats (float4 loads)
        lda = (nc + 3) // 4 * 4
        A32 = numpy.zeros((nc, lda), dtype=numpy.float32)
        A32[:, :nc] = Ainv
        self._keep = (
            device.to_device(agg_ptr.astype(numpy.int32)),
            device.to_device(agg_dofs),
            device.to_device(self.agg_of_host),
            device.to_device(A32),
            )
        k = self._keep
        self.struct = _hip.CoarseS(
            n, nc, _hip.i32(k[0], nc + 1), _hip.i32(k[1], len(agg_dofs)),
            _hip.i32(k[2], n), lda, _hip.f32(k[3], nc * lda)
            )


# -- BLAS-1 / norms -----------------------------------------------------------
def vector_norm(x, kind='l2'):
    lib = _hip.lib()
    code = {'l2': 0, 'linf': 1}[kind]
    res = ctypes.c_double(0.0)
    _hip.check(lib.flow_norm_host(
        x.numel(), _hip.f64(x), code, _hip.f64(work(_hip.REDUCE_WORK)),
        ctypes.byref(res), _hip.stream()
        ))
    return res.value


def dot(x, y):
    lib = _hip.lib()
    assert x.numel() == y.numel()
    res = ctypes.c_double(0.0)
    _hip.check(lib.flow_dot_host(
        x.numel(), _hip.f64(x), _hip.f64(y), _hip.f64(work(_hip.REDUCE_WORK)),
        ctypes.byref(res), _hip.stream()
        ))
    return res.value


def axpby(a, x, b, y):
    '''y = a x + b y'''
    lib = _hip.lib()
    assert x.numel() == y.numel()
    _hip.check(lib.flow_axpby(
        x.numel(), float(a), _hip.f64(x), float(b), _hip.f64(y), _hip.stream()
        ))
    return y


copy = _hip.copy
fill = _hip.fill


def vmul(x, y, out=None, a=1.0):
    '''out = a * x .* y (out may alias x or y)'''
    lib = _hip.lib()
    assert x.numel() == y.numel()
    if out is None:
        out = device.empty(x.numel())
    _hip.check(lib.flow_vmul(
        x.numel(), float(a), _hip.f64(x), _hip.f64(y), _hip.f64(out),
        _hip.stream()
        ))
    return out


# -- Krylov -------------------------------------------------------------------
class StartChooser(object):
    '''Which extrapolation order (1 linear, 2 quadratic) gives a recurring
    solve the better start vector?  Quadratic wins while the fields evolve,
    linear once they only differ by solver noise (which the quadratic weights
    amplify more).  Decided by the iteration counts themselves: the mode in
    use is kept, the other one is tried every `period`-th call.'''

    def __init__(self, period=8):
        self.period = period
        self.calls = 0
        self.mode = 2
        self.its = {}

    def pick(self):
        self.calls += 1
        if self.calls % self.period == 0:
            return 3 - self.mode          # trial of the other mode
        return self.mode

    def report(self, mode, iterations):
        self.its[mode] = iterations
        other = 3 - self.mode
        if other in self.its and self.mode in self.its:
            if self.its[other] < self.its[self.mode] or (
                    self.its[other] == self.its[self.mode] and other == 1):
                self.mode = other


class SolveInfo(object):
    # |Z^T b| / |b| before the projection, of a solve with nullspace= (else
    # None)
    rhs_defect = None

    def __init__(self, iterations, residual, method):
        self.iterations = iterations
        self.residual = residual
        self.method = method

    def __repr__(self):
        return '%s: %d iterations, |r| = %.3e' % (
            self.method, self.iterations, self.residual
            )


def krylov_solve(method, A, b, x, rtol, atol=0.0, maxit=1000, dinv='jacobi',
                 check_every=None, coarse=None, ilu=None, mg=None,
                 first_check=0, tag=None, restart=20, x_is_zero=False,
                 pmg=None, verify=True, guard=None):
    '''Solve A x = b on the device; x holds the initial guess.  Raises
    _hip.NotConverged (a RuntimeError) like dolfin's
    'error_on_nonconvergence'.  first_check > 0: iterations before the first
    residual read-back (then every check_every); the device itself freezes
    the solution at the first iterate that passes the stopping test, so a
    late read-back costs idle launches, never accuracy.  tag (CG): the solve
    recurs in a time loop under that name -- the first read-back comes one
    iteration after the count the previous call (kept on A) needed.
    method 'gmres': GMRES(restart); x_is_zero promises x = 0 on entry;
    `iterations` then counts operator applications (a BiCGStab iteration is
    two); first_check = the applications the caller expects the solve to need
    (that many Arnoldi steps are enqueued before the first read-back);
    verify: check the accepted iterate with the true residual (one more
    operator application; off for the Newton systems, whose outer iteration
    recomputes the nonlinear residual anyway).
    guard (CG): x is a start vector the caller does not vouch for (one
    extrapolated from earlier calls): False / a device vector = its fallback
    (none / that vector).  A start that leaves a larger preconditioned residual
    than zero is dropped on the device for the fallback, and that for zero
    (flow_cg_solve_guarded); `starts_dropped` of the returned info counts.'''
    lib = _hip.lib()
    n = A.size
    if isinstance(dinv, str):
        assert dinv == 'jacobi'
        dinv = A.diag_inv() if ilu is None and pmg is None else None
    assert method in ('cg', 'bicgstab', 'gmres'), method
    nvec = {'cg': 5, 'bicgstab': 7, 'gmres': 2 * restart + 2}[method]
    nparts = A.operator().nblocks * (2 if A.kind == 1 else 1) + 2
    wk = work(_hip.REDUCE_WORK + nvec * n
              + (nparts if method == 'cg' else 0)
              + (2 * coarse.struct.lda if coarse else 0)
              + (2 * max(mg.struct.Ps[0].nblocks, mg.struct.up_nblocks[0])
                 if mg is not None else 0)
              + (n if ilu is not None and method == 'bicgstab' else 0)
              + (_hip.GMRES_PARTIALS + _hip.GMRES_STATE
                 if method == 'gmres' else 0))
    if device._POISON:      # debugging aid: stale workspace reads become NaNs
        _hip.fill(wk, float('nan'))
    if check_every is None:
        check_every = 10 if method == 'bicgstab' else 50
    its = ctypes.c_int(0)
    res = ctypes.c_double(0.0)
    history = None
    if tag is not None and method == 'cg':
        history = A.__dict__.setdefault('_solve_history', {})
        if first_check == 0 and tag in history:
            first_check = history[tag] + 1
    dropped = ctypes.c_int(0)
    if method == 'cg' and guard is not None:
        fallback = None if guard is False else _hip.f64(guard, n, 'x_fallback')
        rc = lib.flow_cg_solve_guarded(
            ctypes.byref(A.operator()), _hip.f64(dinv, n, 'dinv'),
            ctypes.byref(coarse.struct) if coarse is not None else None,
            ctypes.byref(mg.struct) if mg is not None else None,
            _hip.f64(b, n, 'b'), _hip.f64(x, n, 'x'), fallback, float(rtol),
            float(atol), int(maxit), int(check_every), int(first_check),
            _hip.f64(wk), wk.numel(), ctypes.byref(its), ctypes.byref(res),
            ctypes.byref(dropped), _hip.stream()
            )
    elif method == 'cg':
        rc = lib.flow_cg_solve(
            ctypes.byref(A.operator()), _hip.f64(dinv, n, 'dinv'),
            ctypes.byref(coarse.struct) if coarse is not None else None,
            ctypes.byref(mg.struct) if mg is not None else None,
            _hip.f64(b, n, 'b'), _hip.f64(x, n, 'x'), float(rtol), float(atol),
            int(maxit), int(check_every), int(first_check), _hip.f64(wk),
            wk.numel(),
            ctypes.byref(its), ctypes.byref(res), _hip.stream()
            )
    elif method == 'gmres':
        assert coarse is None and mg is None
        rc = lib.flow_gmres_solve(
            ctypes.byref(A.operator()), _hip.f64(dinv, n, 'dinv'),
            ctypes.byref(ilu.struct) if ilu is not None else None,
            ctypes.byref(pmg.struct) if pmg is not None else None,
            _hip.f64(b, n, 'b'), _hip.f64(x, n, 'x'), float(rtol), float(atol),
            int(maxit), int(restart), int(bool(x_is_zero)), int(first_check),
            int(bool(verify)),
            _hip.f64(wk), wk.numel(), ctypes.byref(its), ctypes.byref(res),
            _hip.stream()
            )
    else:
        assert coarse is None and mg is None
        rc = lib.flow_bicgstab_solve(
            ctypes.byref(A.operator()), _hip.f64(dinv, n, 'dinv'),
            ctypes.byref(ilu.struct) if ilu is not None else None,
            _hip.f64(b, n, 'b'), _hip.f64(x, n, 'x'), float(rtol), float(atol),
            int(maxit), int(check_every), int(first_check), _hip.f64(wk),
            wk.numel(),
            ctypes.byref(its), ctypes.byref(res), _hip.stream()
            )
    _hip.check(rc)
    if history is not None:
        history[tag] = its.value
    out = SolveInfo(its.value, res.value,
                    method + ('+2level' if coarse is not None else '')
                    + ('+mg%d' % mg.nlevels if mg is not None else '')
                    + (('+tlilu' if hasattr(ilu, 'cycle') else '+ilu0')
                       if ilu is not None else '')
                    + ('+pmg' if pmg is not None else ''))
    out.starts_dropped = dropped.value
    return out


# -- load vectors, projection, norms -----------------------------------------
def assemble_source(V, f):
    '''(f, v) for v in V (scalar or vector space).'''
    lib = _hip.lib()
    mesh = V.mesh()
    lay = V.layout
    coef = as_cell_coefficient(f, mesh, V.dim)
    cs, keep = coef_struct(coef, mesh, lay.degree)
    b = device.empty(V.size())
    buf = scratch(mesh, V.dim * lay.nloc * mesh.num_cells())
    _hip.check(lib.flow_assemble_source(
        ctypes.byref(mesh_struct(mesh)), ctypes.byref(space_struct(lay)), V.dim,
        ctypes.byref(cs), _hip.f64(buf), _hip.f64(b), _hip.stream()
        ))
    del keep
    return b


def project(f, V, tol=1.0e-14, form_compiler_parameters=None):
    '''L2 projection (dolfin.project): mass solve per component, CG + Jacobi on
    the device.  f: Constant / Expression / Function / NodalExpression, or an
    integrand built from them (flow_amd/fem/forms.py: its load vector comes
    from the form kernels; form_compiler_parameters={'quadrature_degree': q}
    replaces the estimated degree).'''
    from .forms import FormExpr
    if isinstance(f, FormExpr):
        b = form_load_vector(f, V, form_compiler_parameters)
    else:
        b = assemble_source(V, f)
    M = assemble_mass(V)
    dinv = M.diag_inv()
    out = Function(V)
    n = V.N
    for c in range(V.dim):
        x = out.data[c * n:(c + 1) * n]
        krylov_solve('cg', M, b[c * n:(c + 1) * n].contiguous(), x, tol,
                     maxit=1000, dinv=dinv, check_every=10)
    return out


# how the mass systems of the projections below are solved: 'chebyshev' (defect
# correction with a fixed Chebyshev polynomial, flow_amd/fem/mass.py) or 'cg'
MASS_SOLVER = {'method': 'chebyshev', 'steps': 6}


def project_magnitude(u, mode=0, tol=1.0e-12, initial_guess=None):
    '''`project(sqrt(ux**2 + uy**2), FunctionSpace(mesh, 'Lagrange', k))`
    (mode 0; tests/test_karman_vortex_street.py:262-267) or
    `project(abs(ux) + abs(uy), Q)` (mode 1; tests/test_boussinesq.py:268-272)
    for a vector field u of degree k.  `initial_guess`: a previous projection
    to start the mass solve from (step-size controllers call this every step).'''
    from .. import parallel
    lib = _hip.lib()
    W = u.function_space()
    assert W.dim == 2
    mesh = W.mesh()
    lay = W.layout
    S = W.collapse()
    strips = parallel.active()
    # (single GPU: right-hand side and iterate of the mass solve in buffers of
    # the layout -- a loop whose arguments repeat from call to call is replayed
    # as a HIP graph, csrc/graph_replay.hip; the result is copied out)
    # -- only where a replay is possible at all (the option is off by default:
    # the two copies then are not made)
    fixed = not strips and _hip.graphs_possible()
    held = lay._dev.get(('persistent', 'magnitude')) if fixed else None
    if fixed and held is None:
        held = lay._dev[('persistent', 'magnitude')] = (
            device.empty(lay.N), device.empty(lay.N))
    b = _hip.fill(held[0], 0.0) if fixed else device.zeros(lay.N)
    buf = scratch(mesh, lay.nloc * mesh.num_cells())
    _hip.check(lib.flow_assemble_magnitude(
        ctypes.byref(parallel.mesh_view(mesh) if strips else mesh_struct(mesh)),
        ctypes.byref(parallel.view(lay).space if strips else space_struct(lay)),
        int(mode), _hip.f64(u.data, 2 * lay.N), _hip.f64(buf), _hip.f64(b),
        _hip.stream()
        ))
    M = assemble_mass(S)
    key = ('M_dinv',)
    if key not in lay._dev:
        lay._dev[key] = M.diag_inv()
    out = Function(S)
    if initial_guess is not None:
        out.assign(initial_guess)
    tag = 'project_magnitude' if initial_guess is not None else None
    if strips and MASS_SOLVER['method'] == 'chebyshev':
        from .mass import MassSolver
        out.solve_info = parallel.mass_solve(
            MassSolver.cached(M, lay._dev[key], steps=MASS_SOLVER['steps']),
            b, out.data, tol, maxit=100, tag=tag)
    elif strips:
        out.solve_info = parallel.cg(M, lay._dev[key], b, out.data, tol,
                                     maxit=1000, check_every=2, tag=tag)
    elif MASS_SOLVER['method'] == 'chebyshev':
        from .mass import MassSolver
        x = copy(held[1], out.data) if fixed else out.data
        out.solve_info = MassSolver.cached(
            M, lay._dev[key], steps=MASS_SOLVER['steps']).solve(
                b, x, tol, maxit=100, tag=tag)
        if fixed:
            copy(out.data, x)
    else:
        out.solve_info = krylov_solve(
            'cg', M, b, out.data, tol, maxit=1000, dinv=lay._dev[key],
            check_every=2, tag=tag)
    return out


def interpolate(f, V):
    '''f in V: a Function of another space or mesh through fem.Transfer
    (flow_amd/fem/transfer.py), on the GPU; a Constant or an Expression at
    the dof coordinates.'''
    if isinstance(f, Function):
        from .transfer import interpolate_function
        return interpolate_function(f, V)
    out = Function(V)
    if isinstance(f, Constant):
        out.assign(f)
        return out
    assert isinstance(f, Expression)
    vals = f.eval(V.layout.dof_coords.T)
    assert vals.shape[0] == V.dim
    out.set_array(vals.reshape(-1))
    return out


def norm(u, kind='L2'):
    '''norm(Function, 'L2') = sqrt(u^T M u) (tests/test_boussinesq.py:85);
    norm(vector, 'linf'|'l2').'''
    if isinstance(u, Function):
        assert kind == 'L2'
        V = u.function_space()
        M = assemble_mass(V)
        n = V.N
        tmp = device.empty(n)
        total = 0.0
        for c in range(V.dim):
            x = u.data[c * n:(c + 1) * n]
            M.apply(x, tmp)
            total += dot(x, tmp)
        return numpy.sqrt(total)
    data = u.data if hasattr(u, 'data') else u
    return vector_norm(data, kind.lower())


def integral(u):
    '''assemble(u*dx) for a scalar Function: 1^T M u.'''
    V = u.function_space()
    assert V.dim == 1
    M = assemble_mass(V)
    tmp = device.empty(V.N)
    M.apply(u.data, tmp)
    one = torch.ones(V.N, dtype=torch.float64, device=device.get())
    return dot(one, tmp)


def errornorm(exact, uh, degree_rise=3):
    '''L2 error between an Expression and a discrete Function, both
    interpolated per cell into P_(k+degree_rise) as dolfin.errornorm does
    (tests/test_navier_stokes.py:333, 360).  A measurement for the harness:
    evaluated on the host with numpy.'''
    V = uh.function_space()
    mesh = V.mesh()
    k = min(V.degree + degree_rise, 5)
    lat = reference.lattice(k)
    X = cell_lattice_points(mesh, k)                        # (Nc, nl, 2)
    nc, nl = X.shape[:2]
    ue = exact.eval(X.reshape(-1, 2).T).reshape(V.dim, nc, nl)
    tab = reference.tabulate(V.degree, lat)                 # (nl, nloc)
    U = uh.array().reshape(V.dim, V.N)
    uhl = numpy.einsum('acj,lj->acl', U[:, V.layout.cell_dofs], tab)
    e = ue - uhl
    Mk = reference.mass_matrix(k)
    detj = 2.0 * mesh.cell_areas()
    return float(numpy.sqrt(numpy.einsum('acl,lm,acm,c->', e, Mk, e, detj)))


# -- forms (flow_amd/fem/forms.py, csrc/form_kernels.hip) ---------------------
_FORM_TABLES = {}


def _form_tables(q, expr_degrees, facet=False, scheme='default'):
    '''Rule (nq x 3: xi, eta, weight; on facets 3*nq rows, the points of
    local facets 0, 1, 2: reference.facet_rule) and the P_k basis tables of
    the Expression operands at its points, uploaded once per (degree, lattice
    degrees, cells | facets): an upload drains the stream, and time loops
    integrate the same forms every step.  (The program and the constants
    need no upload: they travel with the launch.)  Returns (rule, tables,
    table offsets, nq per cell or facet, doubles in tables).  scheme
    'vertex' (cells only): the cell vertices with weights |T|/3, whatever
    q.'''
    if scheme == 'vertex':
        if facet:
            raise ValueError('the vertex quadrature rule is defined on cells')
        q = None
    key = (q, expr_degrees, facet, str(device.get()))
    held = _FORM_TABLES.get(key)
    if held is None:
        if scheme == 'vertex':
            pts = numpy.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]])
            rule = numpy.concatenate([pts, numpy.full((3, 1), 1.0 / 6.0)],
                                     axis=1)
            nq = 3
        elif facet:
            rule = reference.facet_rule(q)
            pts = rule[:, :2]
            nq = len(rule) // 3
        else:
            pts, wts = reference.triangle_rule(q)
            rule = numpy.concatenate([pts, wts[:, None]], axis=1)
            nq = len(wts)
        if len(rule) > _hip.FORM_MAX_POINTS:
            raise ValueError('quadrature degree %d: %d points, the limit is %d'
                             % (q, len(rule), _hip.FORM_MAX_POINTS))
        offsets = []
        tabs = [numpy.zeros(1)]
        off = 1
        for k in expr_degrees:
            t = reference.tabulate(k, pts)              # (points, nl)
            offsets.append(off)
            tabs.append(t.reshape(-1))
            off += t.size
        tables = numpy.concatenate(tabs)
        held = (device.to_device(rule.reshape(-1).copy()),
                device.to_device(tables), offsets, nq, int(tables.size))
        if len(_FORM_TABLES) >= 64:
            _FORM_TABLES.clear()
        _FORM_TABLES[key] = held
    return held


def _form_struct(prog, mesh, q, facet=False, scheme='default'):
    '''flow_form of a compiled forms.Program on `mesh` with the degree-q
    rule of the cells, or of the facets (scheme 'vertex': the vertex rule of
    the cells).  Returns (struct, keepalive).'''
    fs = _hip.FormS()
    fs.nprog = len(prog.code)
    # (a field of a ctypes struct is a new view at every access: taken once)
    code = fs.prog
    for i, ins in enumerate(prog.code):
        code[4 * i], code[4 * i + 1], code[4 * i + 2], code[4 * i + 3] = \
            int(ins[0]), int(ins[1]), int(ins[2]), int(ins[3])
    fs.nconst = _refresh_constants(prog, fs.consts)
    keep = []
    nc = mesh.num_cells()
    fs.nfield = len(prog.fields)
    for i, (f, comp) in enumerate(prog.fields):
        W = f.function_space()
        if W.mesh() is not mesh:
            raise ValueError('a field of the integrand lives on another mesh')
        lay = W.layout
        base = _hip.f64(f.data, W.size(), 'field of the integrand').value
        fs.field[i] = base + 8 * comp * lay.N
        fs.field_deg[i] = lay.degree
        fs.cell_dofs[lay.degree - 1] = _hip.i32(
            lay.dev('cell_dofs'), lay.nloc * nc, 'cell_dofs').value
        keep.append(f.data)
    expr_degrees = tuple(int(e.degree) for e, _ in prog.exprs)
    rule, tables, offsets, nq, ntables = _form_tables(q, expr_degrees, facet,
                                                      scheme)
    fs.nexpr = len(prog.exprs)
    coefs = {}
    for i, (e, comp) in enumerate(prog.exprs):
        if id(e) not in coefs:
            # (a coefficient with a lattice of its own, stabilization.SupgTau:
            # computed on the device now, from its field's current values)
            coefs[id(e)] = e.form_lattice(mesh) if hasattr(e, 'form_lattice') \
                else as_cell_coefficient(e, mesh, e.value_dim())
        coef = coefs[id(e)]
        n = coef.nl * nc
        base = _hip.f64(coef.values, coef.dim * n, 'Expression lattice').value
        fs.expr[i] = base + 8 * comp * n
        fs.expr_nl[i] = coef.nl
        fs.expr_table[i] = offsets[i]
        keep.append(coef.values)
    fs.nq = nq
    fs.rule = _hip.f64(rule, (9 if facet else 3) * nq, 'rule').value
    fs.tables = _hip.f64(tables, ntables, 'tables').value
    fs.ntables = ntables
    fs.nout = prog.nout
    return fs, (keep, rule, tables)


def _no_strips(what):
    from .. import parallel
    if parallel.active():
        raise NotImplementedError(
            '%s on strips is not implemented (project_magnitude is the path '
            'there)' % what)


def assemble(form, form_compiler_parameters=None):
    '''By the rank of the form.  0: assemble(f*dx), assemble(f*ds(k)) and
    signed sums of such forms -- the integral of a scalar integrand over the
    cells or the exterior facets of the mesh, a float.  1: forms of a
    TestFunction, a Vector.  2: forms of a TrialFunction and a TestFunction,
    a Matrix of kind 0 on the space's pattern.  Arguments of a vector space
    (forms.vector_arguments(True) allows them): a Vector of 2N, a Matrix of
    kind 2.  Ranks 1 and 2 go part by part through _assemble_arguments (on a
    vector space _block_part) and the launches of _launch_dx /
    _launch_block_dx, which NewtonAssembler issues too.  Parts of rank 1 and 2
    over ds (Neumann, Robin, Nitsche terms: forms.facet_arguments(True)
    allows them) go through flow_form_facet_vector / flow_form_facet_matrix
    and the facet contribution map (facet_map); an empty selection, ds(99),
    contributes zero.  The parts of a sum are assembled one by one, each at
    its own degree, and added in the order written; fixed-order reductions
    and gathers on the device: the same bits on every call.
    form_compiler_parameters: 'quadrature_degree' replaces the estimate (a
    measure's own metadata comes first), 'quadrature_rule': 'vertex' selects
    the vertex rule for ranks 1 and 2 (functionals do not read that key).'''
    from . import forms
    if not isinstance(form, forms.Form):
        raise TypeError('assemble takes a form, f*dx or f*ds (got %r)'
                        % (type(form),))
    _no_strips('assemble')
    rank = form.rank
    if rank > 0:
        return _assemble_arguments(form, rank, form_compiler_parameters)
    if isinstance(form, forms.FormSum):
        total = 0.0
        for sign, part in form.terms():
            total += sign * assemble(part, form_compiler_parameters)
        return total
    q = _form_degree(form, form_compiler_parameters)
    lib = _hip.lib()
    mesh = forms.form_mesh(form.integrand, form.mesh)
    if form.integral_type == 'interior_facet':
        fs, keep, sel = _interior_facet_job(form, mesh, q)
        if sel.count == 0:          # (dS(99): exactly 0.0, nothing launched)
            return 0.0
        res = ctypes.c_double(0.0)
        _hip.check(lib.flow_form_interior_facet_functional(
            ctypes.byref(mesh_struct(mesh)), ctypes.byref(fs), sel.count,
            _hip.i32(sel.plus, sel.count, 'facet + cells'),
            _hip.i32(sel.local, sel.count, 'facet + local indices'),
            _hip.i32(sel.other, sel.count, 'facet - cells'),
            _hip.f64(scratch(mesh, max(sel.count, 1))),
            _hip.f64(work(_hip.REDUCE_WORK)), ctypes.byref(res), _hip.stream()
            ))
        del keep
        return res.value
    facet = form.integral_type == 'exterior_facet'
    prog = forms.compile_trees([form.integrand.comps], facet=facet)
    fs, keep = _form_struct(prog, mesh, q, facet)
    res = ctypes.c_double(0.0)
    if is_cell_subdomain(form):
        cells, nsel = cell_lists(mesh, form.subdomain_data, form.subdomain_id)
        if nsel == 0:               # (dx(99): exactly 0.0, nothing launched)
            return 0.0
        _hip.check(lib.flow_form_cells_functional(
            ctypes.byref(mesh_struct(mesh)), ctypes.byref(fs), nsel,
            _hip.i32(cells, nsel, 'cell list'),
            _hip.f64(scratch(mesh, nsel)),
            _hip.f64(work(_hip.REDUCE_WORK)), ctypes.byref(res), _hip.stream()
            ))
    elif facet:
        cells, local, nf = facet_lists(mesh, form.subdomain_data,
                                       form.subdomain_id)
        _hip.check(lib.flow_form_facet_functional(
            ctypes.byref(mesh_struct(mesh)), ctypes.byref(fs), nf,
            _hip.i32(cells, nf, 'facet cells'),
            _hip.i32(local, nf, 'facet local indices'),
            _hip.f64(scratch(mesh, max(nf, 1))),
            _hip.f64(work(_hip.REDUCE_WORK)), ctypes.byref(res), _hip.stream()
            ))
    else:
        _hip.check(lib.flow_form_functional(
            ctypes.byref(mesh_struct(mesh)), ctypes.byref(fs),
            _hip.f64(scratch(mesh, mesh.num_cells())),
            _hip.f64(work(_hip.REDUCE_WORK)), ctypes.byref(res), _hip.stream()
            ))
    del keep
    return res.value


def _assemble_arguments(form, rank, form_compiler_parameters=None):
    '''assemble() of a form, or of a signed sum of forms, of rank 1 (a
    Vector) or 2 (a Matrix; on a vector space a vector of 2N, a Matrix of
    kind 2), part by part: the programs of a part are compiled while the
    kernels of the part before run.  Scalar space: _scalar_part; vector
    space: _block_part.  The first result of sign +1 IS the total, ds
    included.'''
    from . import forms
    from .function import Vector
    V = form.arguments()[0]
    if forms.is_mixed_space(V):
        # (a Taylor-Hood space, forms.mixed_arguments: a MixedMatrix or a
        # Vector of 2 Nv + Np)
        from . import mixed
        return mixed.assemble_form(form, rank, form_compiler_parameters)
    lay, mesh = V.layout, V.mesh()
    total = _Sum()
    for sign, part in form.terms():
        _check_part_mesh(part, mesh)
        _, table = part.argument_table()
        q, scheme = _part_rule(part, form_compiler_parameters)
        if V.dim == 2:
            total.add(sign, _block_part(part, table, rank, q, scheme, lay,
                                        mesh), True)
        else:
            _scalar_part(part, table, rank, q, scheme, lay, mesh, total, sign)
    if total.total is None:
        raise ValueError('an empty sum of forms has no rank')
    if rank == 2:
        return Matrix(lay, 2 if V.dim == 2 else 0, total.total)
    return Vector(total.total)


def _scalar_part(part, table, rank, q, scheme, lay, mesh, total, sign):
    '''One part of a form of arguments on a scalar space (a scalar form's, or
    the pressure corner of a mixed form's: mixed.assemble_form) into the sum
    `total`: one launch per program -- one program, or several whose results
    add up where the table exceeds the limits of flow_form
    (forms.argument_programs) --, each result added at once.  dx: _launch_dx;
    a ds or dx(k) part: _selection_arguments into a zeroed buffer (the gather
    writes its targets only: the rest stays zero).'''
    from . import forms
    facet = part.integral_type == 'exterior_facet'
    for prog in forms.argument_programs(table, rank, facet):
        fs, keep = _form_struct(prog, mesh, q, facet, scheme)
        if facet or is_cell_subdomain(part):
            out = value_plane(lay) if rank == 2 else device.zeros(lay.N)
            _selection_arguments(mesh, lay, rank, fs, part, out)
        elif rank == 2:
            out = value_plane(lay)
            _launch_dx(mesh, lay, 'matrix', fs, out, None)
        else:
            out = device.empty(lay.N)
            _launch_dx(mesh, lay, 'vector', fs, None, out)
        del keep
        total.add(sign, out, True)


def _block_part(part, table, rank, q, scheme, lay, mesh):
    '''One part of a form of arguments on a vector space into a fresh buffer:
    four planes (rank 2; plane 2 r + s the block of test component r and
    trial component s) or a vector of 2N.  A dx part is ONE block launch with
    the programs of all its blocks (_launch_block_dx); a ds part, and a
    dx(k) part, goes block by block, program by program, through
    _selection_arguments with the scalar layout's facet_map / cell_map into
    the block's plane or component (a further program of a block into a
    zeroed buffer of its own, then added).'''
    from . import forms
    facet = part.integral_type == 'exterior_facet'
    stride = plane_stride(lay) if rank == 2 else lay.N
    nblocks = 4 if rank == 2 else 2
    progs = [(p, prog) for p, block in forms.block_items(table, rank)
             for prog in forms.argument_programs(block, rank, facet)]
    tags = tuple(p for p, _ in progs)
    structs, keeps = _program_structs(
        [(prog, q, scheme, facet) for _, prog in progs], mesh)
    if not facet and not is_cell_subdomain(part):
        out = device.empty(nblocks * stride)
        if rank == 2 and stride != lay.nnz:   # (the entry behind every plane)
            _hip.fill(out, 0.0)
        _launch_block_dx(mesh, lay, structs,
                         ('matrix' if rank == 2 else 'vector',) * len(tags),
                         tags, out if rank == 2 else None, stride,
                         out if rank == 1 else None)
        return out
    # (the facet gather writes its targets only: the rest stays zero)
    out = device.zeros(nblocks * stride)
    width = lay.nnz if rank == 2 else lay.N
    for k, p in enumerate(tags):
        dst = out[p * stride:p * stride + width]
        tmp = device.zeros(width) if p in tags[:k] else dst
        _selection_arguments(mesh, lay, rank, structs[k], part, tmp)
        if tmp is not dst:
            axpby(1.0, tmp, 1.0, dst)
    return out


def _scalar_bcs(bcs, V):
    '''(dofs, values) on the device and the byte mask of the Dirichlet dofs
    of conditions on the space V (None, None, None without any).  V scalar:
    conditions on V, a mask of N bytes.  V a vector space: conditions on V
    and on V.sub(i), dofs in operator numbering (a*N + i), a mask of 2N
    bytes.'''
    from .bcs import collect
    if bcs is None:
        bcs = []
    if not isinstance(bcs, (list, tuple)):
        bcs = [bcs]
    for bc in bcs:
        W = bc.function_space()
        if V.dim == 2 and W.component is not None:
            W = W.parent
        elif W.component is not None:
            W = None
        if W is None or not W.same_as(V):
            raise ValueError('a Dirichlet condition lives on another space '
                             'than the form')
    dofs, vals = collect(list(bcs), V.size())
    if len(dofs) == 0:
        return None, None, None
    mask = numpy.zeros(V.size(), dtype=numpy.uint8)
    mask[dofs] = 1
    return (device.to_device(dofs), device.to_device(vals),
            device.to_device(mask))


def _set_values(dofs, vals, x):
    _hip.check(_hip.lib().flow_bc_set_values(
        dofs.numel(), _hip.i32(dofs), _hip.f64(vals, dofs.numel()),
        _hip.f64(x), _hip.stream()))


def _form_space(a):
    found = a.arguments()
    if a.rank != 2:
        raise ValueError('the left-hand side must be a bilinear form (rank 2)')
    return found[0]


def assemble_system(a, L, bcs=None, form_compiler_parameters=None):
    '''(A, b) of the bilinear form a and the linear form L (None or an empty
    sum: zero) with dolfin's symmetric elimination of the Dirichlet
    conditions: rows and columns of their dofs are zeroed, the diagonal is 1,
    b is lifted by the eliminated columns and b[dof] = g.  Forms on a vector
    space W: A of kind 2, b of 2N, conditions on W and on W.sub(i)
    (flow_bc_symmetric_blocks).'''
    from . import forms
    from .function import Vector
    _no_strips('assemble_system')
    V = _form_space(a)
    if forms.is_mixed_space(V):
        from . import mixed
        return mixed.assemble_system(a, L, bcs, form_compiler_parameters)
    A0 = assemble(a, form_compiler_parameters)
    if L is None or (isinstance(L, forms.FormSum) and not L.terms()):
        b = Vector(device.zeros(V.size()))
    else:
        if L.rank != 1:
            raise ValueError('the right-hand side must be a linear form '
                             '(rank 1)')
        if not L.arguments()[0].same_as(V):
            raise NotImplementedError('test functions of different spaces or '
                                      'meshes on the two sides')
        b = assemble(L, form_compiler_parameters)
    dofs, vals, mask = _scalar_bcs(bcs, V)
    if dofs is None:
        return A0, b
    g = device.zeros(V.size())
    _set_values(dofs, vals, g)
    lift = A0.apply(g, device.empty(V.size()))
    axpby(-1.0, lift, 1.0, b.data)
    _set_values(dofs, vals, b.data)
    if A0.kind == 2:
        return symmetric_bc_blocks(A0, mask), b
    return symmetric_bc_matrix(A0, mask), b


def apply_identity_rows(bc, A=None, b=None):
    '''DirichletBC.apply: the rows of the condition's dofs of A become
    identity rows, the entries of b its values (no column elimination).
    Not on strips (the steppers apply their conditions themselves there).'''
    _no_strips('DirichletBC.apply')
    V = bc.function_space()
    if V.component is not None or V.dim == 2:
        # a condition on W or W.sub(i): a kind-2 matrix, vectors of 2N
        V = V.parent if V.component is not None else V
        kind = 2
    else:
        kind = 0
    dofs, vals, _ = _scalar_bcs([bc], V)
    if dofs is None:
        return
    if A is not None:
        if A.kind != kind or A.layout is not V.layout:
            raise ValueError('the matrix does not belong to the space of the '
                             'condition')
        _hip.check(_hip.lib().flow_bc_identity_rows(
            ctypes.byref(A.operator()), _hip.f64(A.vals),
            _hip.i32(V.layout.dev('diag_idx')), dofs.numel(), _hip.i32(dofs),
            _hip.stream()))
    if b is not None:
        data = b.data if hasattr(b, 'data') else b
        if data.numel() != V.size():
            raise ValueError('the vector does not belong to the space of the '
                             'condition')
        _set_values(dofs, vals, data)


_KRYLOV_METHODS = ('cg', 'gmres', 'bicgstab')


def _solve_cg_nullspace(A, b, u, ns, prm, ks):
    '''The CG route of solve(a == L, ..., nullspace=ns) on a scalar or vector
    space, after nullspace.validate: b projected, the native CG untouched, u
    projected; the returned SolveInfo carries rhs_defect.'''
    from . import nullspace
    nullspace.check_null(ns, A, prm.get('nullspace_check'))
    slots = ns.project_rhs(b.data)
    ns.deflate(u.data)
    info = krylov_solve(
        'cg', A, b.data, u.data, ks.get('relative_tolerance', 1.0e-12),
        atol=ks.get('absolute_tolerance', 0.0),
        maxit=int(ks.get('maximum_iterations', 1000)), check_every=10)
    ns.deflate(u.data)
    info.rhs_defect = ns.defect(slots)
    return info


def solve(equation, u, bcs=None, J=None, solver_parameters=None,
          form_compiler_parameters=None, nullspace=None):
    '''solve(F == 0, u, bcs, J=None): Newton's method, newton_solve below
    (J: the Jacobian, derivative(F, u) by default; for a linear equation it
    must stay None).
    solve(a == L, u, bcs): assemble_system, then a Krylov solve on the
    device that starts from u's values and writes into u.  Returns the
    SolveInfo.  The form counts as symmetric where every part of a is
    structurally symmetric, or where solver_parameters['symmetric'] is True.
    solver_parameters: 'linear_solver' 'cg' | 'gmres' | 'bicgstab'; absent,
    'default' or 'iterative': CG for a symmetric form, else GMRES.  The
    preconditioner follows one rule, whether the method was chosen or
    defaulted: ILU(0) iff the method is not CG and the form is not symmetric,
    Jacobi otherwise -- so 'gmres' or 'bicgstab' on a symmetric form run with
    Jacobi, and 'cg' on a non-symmetric form is run as asked, with Jacobi and
    without a warning (it may not converge: NotConverged).  'krylov_solver':
    'relative_tolerance' (1e-12), 'absolute_tolerance' (0),
    'maximum_iterations' (1000).  There is no direct solver.  A pure Neumann
    problem is singular: pass its nullspace.  Raises _hip.NotConverged (a
    RuntimeError).  Not on strips.
    nullspace: a fem.VectorSpaceBasis (fem/nullspace.py: constant_nullspace,
    rigid_body_modes) of the singular operator, orthonormal; None: nothing
    changes.  The left and the right nullspace must coincide (one basis
    serves both; not checked).  Scalar and vector spaces: the CG route only
    (a symmetric form, Jacobi) -- b is projected, the native CG runs
    untouched, u is projected; the ILU(0) routes and Newton's method on these
    spaces are a NotImplementedError.  Taylor-Hood spaces: MINRES, FGMRES and
    Newton's method (fem/mixed.py).  Before the solve: the basis must be
    orthonormal, live on the space of the unknown, vanish on the Dirichlet
    dofs, and satisfy |A z|_inf <= sqrt(eps) |A|_inf |z|_inf (the threshold:
    solver_parameters['nullspace_check']; False skips it) -- each a
    ValueError.  The returned info carries rhs_defect = |Z^T b| / |b| from
    before the projection: an inconsistent right-hand side (the integral of f
    not 0) shows there.'''
    from . import forms
    _no_strips('solve')
    if not isinstance(equation, forms.Equation):
        raise TypeError('solve takes an equation a == L of a bilinear and a '
                        'linear form (got %r)' % (type(equation),))
    if isinstance(equation.rhs, numbers.Real):
        if isinstance(u, Function) and forms.is_mixed_space(
                u.function_space()):
            if forms.mixed_derivatives.enabled:
                # (Newton on a Taylor-Hood space: fem/mixed.py)
                from . import mixed
                return mixed.newton_solve(equation.lhs, u, bcs, J,
                                          solver_parameters,
                                          form_compiler_parameters, nullspace)
            raise NotImplementedError(
                'solve(F == 0) on a mixed space: Newton\'s method takes '
                'scalar and vector spaces only')
        if nullspace is not None:
            raise NotImplementedError(
                'nullspace= with Newton\'s method on a scalar or vector '
                'space (Taylor-Hood spaces take it)')
        return newton_solve(equation.lhs, u, bcs, J, solver_parameters,
                            form_compiler_parameters)
    if J is not None:
        raise ValueError('J= belongs to the nonlinear solve(F == 0, u, ...)')
    prm = dict(solver_parameters or {})
    method = prm.get('linear_solver', 'default')
    if method not in _KRYLOV_METHODS + ('default', 'iterative'):
        raise ValueError(
            'linear_solver %r: there is no direct solver here; the choices '
            'are %s' % (method, ', '.join(_KRYLOV_METHODS + ('default',))))
    a, L = equation.lhs, equation.rhs
    V = _form_space(a)
    if forms.is_mixed_space(V):
        # (symmetric forms only: preconditioned MINRES, fem/mixed.py)
        from . import mixed
        return mixed.solve(a, L, u, bcs, solver_parameters,
                           form_compiler_parameters, nullspace)
    if not isinstance(u, Function) or not u.function_space().same_as(V):
        raise ValueError('solve writes into a Function of the space of the '
                         'trial function')
    symmetric = prm.get('symmetric') is True or all(
        forms.is_symmetric_table(part.argument_table()[1])
        for _, part in a.terms())
    if method in ('default', 'iterative'):
        method = 'cg' if symmetric else 'gmres'
    ks = dict(prm.get('krylov_solver') or {})
    if nullspace is not None and method != 'cg':
        raise NotImplementedError(
            'nullspace= on a scalar or vector space takes the CG route (a '
            "symmetric form with Jacobi); %r%s is not built for a singular "
            'matrix' % (method, '' if symmetric else ' with ILU(0)'))
    if nullspace is not None:
        from . import nullspace as nsp
        from .bcs import collect
        held = [] if bcs is None else (
            list(bcs) if isinstance(bcs, (list, tuple)) else [bcs])
        nsp.validate(nullspace, V, collect(held, V.size())[0])
    A, b = assemble_system(a, L, bcs, form_compiler_parameters)
    if nullspace is not None:
        return _solve_cg_nullspace(A, b, u, nullspace, prm, ks)
    ilu = None
    if method != 'cg' and not symmetric:
        from .ilu import Ilu0
        ilu = Ilu0(A)
    info = krylov_solve(
        method, A, b.data, u.data, ks.get('relative_tolerance', 1.0e-12),
        atol=ks.get('absolute_tolerance', 0.0),
        maxit=int(ks.get('maximum_iterations', 1000)), ilu=ilu,
        check_every=10)
    return info


# -- Newton's method: solve(F == 0, u, bcs, J) ----------------------------------
NEWTON_DEFAULTS = {
    'maximum_iterations': 50, 'relative_tolerance': 1.0e-9,
    'absolute_tolerance': 1.0e-10, 'relaxation_parameter': 1.0,
    'error_on_nonconvergence': True, 'convergence_criterion': 'residual',
    'report': False, 'linear_solver': 'default', 'krylov_solver': None,
    }


def newton_parameters(solver_parameters):
    '''(newton_solver dict with dolfin's defaults filled in, symmetric flag)
    of the solver_parameters of solve(F == 0, ...); ValueError for what is
    not built ('snes', the 'incremental' criterion, direct solvers) and for
    unknown keys.  Needs no device.'''
    prm = dict(solver_parameters or {})
    unknown = set(prm) - {'nonlinear_solver', 'newton_solver', 'symmetric'}
    if unknown:
        raise ValueError('solver_parameters of a nonlinear solve: unknown '
                         'keys %s' % sorted(unknown))
    if prm.get('nonlinear_solver', 'newton') != 'newton':
        raise ValueError("nonlinear_solver %r: only 'newton' is built"
                         % (prm['nonlinear_solver'],))
    given = dict(prm.get('newton_solver') or {})
    unknown = set(given) - set(NEWTON_DEFAULTS)
    if unknown:
        raise ValueError('newton_solver: unknown keys %s' % sorted(unknown))
    ns = dict(NEWTON_DEFAULTS)
    ns.update(given)
    if ns['convergence_criterion'] != 'residual':
        raise ValueError("convergence_criterion %r: only 'residual' is built"
                         % (ns['convergence_criterion'],))
    if ns['linear_solver'] not in _KRYLOV_METHODS + ('default', 'iterative'):
        raise ValueError(
            'linear_solver %r: there is no direct solver here; the choices '
            'are %s' % (ns['linear_solver'],
                        ', '.join(_KRYLOV_METHODS + ('default',))))
    ns['krylov_solver'] = dict(ns['krylov_solver'] or {})
    return ns, prm.get('symmetric') is True


class NewtonInfo(object):
    '''What solve(F == 0, ...) returns: `iterations` (linear solves done),
    `converged`, `residuals` (|F|_2 before the first and after every
    iteration), `linear_iterations` (of every linear solve), `fused` (every
    dx part of the Jacobian was assembled together with a part of the
    residual by flow_form_newton; ds parts are never fused and do not count:
    they go through flow_form_facet_matrix / flow_form_facet_vector one by
    one; on a vector space: there is a 'newton' job, no dx component of the
    residual needed a 'vector' job and no block of a fused row was split into
    several programs -- block_jobs_fused), `method` (of the linear solves),
    `route` (NewtonAssembler.route: 'by_parts' where a ds or dx(k) part is
    gathered on its own, else 'fused' | 'pair'), `frozen` (on a Taylor-Hood
    space, mixed.newton_solve: the blocks of the Jacobian, in
    MixedMatrix.blocks() naming, that do not read the unknown and were
    assembled once; () elsewhere), `rhs_defect` (with nullspace=: the largest
    |Z^T F| / |F| over the linear solves, taken before the projection; else
    None).'''
    frozen = ()
    rhs_defect = None

    def __init__(self, fused, method, route=None):
        self.iterations = 0
        self.converged = False
        self.residuals = []
        self.linear_iterations = []
        self.fused = fused
        self.method = method
        self.route = route or ('fused' if fused else 'pair')

    def __repr__(self):
        return 'newton (%s, %s): %d iterations, |F| = %.3e, %s' % (
            self.method, 'fused' if self.fused else 'pair', self.iterations,
            self.residuals[-1] if self.residuals else float('nan'),
            'converged' if self.converged else 'NOT converged')


def _part_rule(part, form_compiler_parameters):
    '''(degree, scheme) a part of a form of arguments is integrated with.'''
    from . import forms
    q = forms._quadrature_degree(part.metadata)
    if q is None:
        q = forms._quadrature_degree(form_compiler_parameters)
    q = forms.check_degree(part.degree() if q is None else q)
    scheme = forms.quadrature_scheme(form_compiler_parameters, part.metadata)
    if scheme == 'vertex' and part.integral_type == 'exterior_facet':
        raise ValueError("quadrature_rule 'vertex' on a ds part with test or "
                         "trial functions: the vertex rule is a rule of cells")
    return q, scheme


def _check_part_mesh(part, mesh):
    from . import forms
    if forms.form_mesh(part.integrand, part.mesh) is not mesh:
        raise ValueError('the form is integrated over another mesh than the '
                         'one of its arguments')


# -- the jobs of an assembly --------------------------------------------------
# One launch's worth of one Program.  kind: 'newton' | 'matrix' | 'vector' |
# 'facet_matrix' | 'facet_vector' | 'cells_matrix' | 'cells_vector'; msign,
# vsign: the signs of the matrix and of the vector part (0.0 where the kind has
# none); part: the ds part of a facet job or the dx(k) part of a cells job (its
# subdomain data and id are the selection), else None; tag: the block plane
# p = 2 r + s ('newton', 'matrix', 'facet_matrix', 'cells_matrix') or the
# component r ('vector', 'facet_vector', 'cells_vector') on a vector space -- a
# 'newton' job assembles
# block p and component p // 2 --, 0 on a scalar space; call: (index of the
# part of J or None, index of the part of F or None).
Job = collections.namedtuple(
    'Job', 'kind msign vsign program degree scheme part tag call')


def _block_rows(tj, tf, dim=2):
    '''The dx jobs [(kind, Program, tag)] of one part of J (block table tj)
    taken together with one part of F (block table tf), row by row (r = the
    test component): block (r, s) and component r fuse into a 'newton' job
    (tag p = dim r + s) where forms.newton_program fits the limits of
    flow_form, s = r first, else the other block of the row; the other blocks
    of the row are 'matrix' jobs (tag p), a component that did not fuse
    'vector' jobs (tag r), program by program (forms.argument_programs).  A
    scalar space (dim 1) is the single row of the single block.'''
    from . import forms
    if dim == 1:
        tj, tf = [[tj]], [tf]
    rows = []
    for r in range(dim):
        fused = None
        if tf[r] is not None:
            for s in [r] + [s for s in range(dim) if s != r]:
                if tj[r][s] is None:
                    continue
                try:
                    fused = (s, forms.newton_program(tj[r][s], tf[r]))
                    break
                except ValueError:      # over a limit of flow_form
                    continue
        if fused is not None:
            rows.append(('newton', fused[1], dim * r + fused[0]))
        for s in range(dim):
            if tj[r][s] is not None and (fused is None or s != fused[0]):
                rows.extend(('matrix', prog, dim * r + s)
                            for prog in forms.argument_programs(tj[r][s], 2))
        if tf[r] is not None and fused is None:
            rows.extend(('vector', prog, r)
                        for prog in forms.argument_programs(tf[r], 1))
    return rows


def newton_jobs(J, F, form_compiler_parameters=None, fuse=True):
    '''The launches that assemble (J, F) at one state, as a list of Job
    records, on a scalar space (one block, tag 0) and on a vector space
    alike.  ds parts are never fused: 'facet_matrix' / 'facet_vector' jobs
    block by block, program by program; dx(k) parts neither: 'cells_matrix' /
    'cells_vector' jobs in the same way.  A dx part of J is taken together
    with the first unused dx part of F of the same degree and rule (the one it
    was derived from first) with which at least one row fuses (_block_rows);
    without one, and with fuse=False, its blocks are 'matrix' jobs and the
    parts of F 'vector' jobs, in the order written: the pair assemble(J),
    assemble(F).  The dx jobs of one call on a vector space are ONE launch of
    flow_form_block_newton (both indices), flow_form_block_matrix or
    flow_form_block_vector; on a scalar space every job is a launch
    (flow_form_newton / flow_form_matrix / flow_form_vector).  Host only.'''
    from . import forms
    dim = F.arguments()[0].dim
    # [(tag, table)] of the present blocks of a part's table; a scalar space
    # is the 1 x 1 case: the table itself, tag 0
    blocks = forms.block_items if dim == 2 else lambda table, rank: [(0, table)]
    jparts, fparts = J.terms(), F.terms()
    rules = [_part_rule(p, form_compiler_parameters) for _, p in fparts]
    used = [False] * len(fparts)
    jobs = []
    for ji, (sj, pj) in enumerate(jparts):
        rule = _part_rule(pj, form_compiler_parameters)
        tj = pj.argument_table()[1]
        if pj.integral_type == 'exterior_facet' or is_cell_subdomain(pj):
            # (a part over a selection is never fused)
            facet = pj.integral_type == 'exterior_facet'
            jobs.extend(Job('facet_matrix' if facet else 'cells_matrix', sj,
                            0.0, prog, rule[0], rule[1], pj, p, (ji, None))
                        for p, block in blocks(tj, 2)
                        for prog in forms.argument_programs(block, 2, facet))
            continue
        fi, rows = None, None
        origin = getattr(pj, 'derived_from', None)
        for i in sorted(range(len(fparts)),
                        key=lambda i: fparts[i][1] is not origin):
            if not fuse or used[i] or rules[i] != rule \
                    or fparts[i][1].integral_type != 'cell' \
                    or is_cell_subdomain(fparts[i][1]):
                continue
            found = _block_rows(tj, fparts[i][1].argument_table()[1], dim)
            if any(kind == 'newton' for kind, _, _ in found):
                fi, rows = i, found
                break
        if fi is None:
            rows = [('matrix', prog, p) for p, block in blocks(tj, 2)
                    for prog in forms.argument_programs(block, 2)]
        else:
            used[fi] = True
        sf = 0.0 if fi is None else fparts[fi][0]
        jobs.extend(Job(kind, 0.0 if kind == 'vector' else sj,
                        0.0 if kind == 'matrix' else sf, prog, rule[0],
                        rule[1], None, tag, (ji, fi))
                    for kind, prog, tag in rows)
    for i, (sf, pf) in enumerate(fparts):
        facet = pf.integral_type == 'exterior_facet'
        cells = is_cell_subdomain(pf)
        if used[i]:
            continue
        jobs.extend(Job('facet_vector' if facet else
                        'cells_vector' if cells else 'vector', 0.0, sf, prog,
                        rules[i][0], rules[i][1],
                        pf if facet or cells else None, r, (None, i))
                    for r, block in blocks(pf.argument_table()[1], 1)
                    for prog in forms.argument_programs(block, 1, facet))
    return jobs


# NewtonInfo.fused: two rules, on purpose.  On a scalar space a job list is
# fused where no dx part of J needed a 'matrix' job; on a vector space a fused
# row keeps 'matrix' jobs (its other block), so the rule there asks for more.
def _scalar_jobs_fused(jobs):
    '''NewtonInfo.fused of jobs on a scalar space: every dx part of J went
    into a 'newton' job.  ds jobs do not count; a dx(k) job is never fused.'''
    return all(j.kind not in ('matrix', 'cells_matrix', 'cells_vector')
               for j in jobs)


def block_jobs_fused(jobs):
    '''NewtonInfo.fused of jobs on a vector space: there is a 'newton' job, no
    dx residual component needed a 'vector' job, and every block of a row that
    has a 'newton' job in its call is ONE program (no table of such a row was
    split).  ds jobs do not count.'''
    if not any(j.kind == 'newton' for j in jobs) \
            or any(j.kind in ('vector', 'cells_matrix', 'cells_vector')
                   for j in jobs):
        return False
    for j in jobs:
        if j.kind != 'newton':
            continue
        row = [k.tag for k in jobs if k.call == j.call
               and k.kind in ('newton', 'matrix') and k.tag // 2 == j.tag // 2]
        if len(row) != len(set(row)):
            return False
    return True


# -- the launch layer: all size arithmetic, ctypes packing and _hip.check -----
_BLOCK_KINDS = {'newton': 0, 'matrix': 1, 'vector': 2}     # include/flow_hip.h


def _block_newton_scratch(kinds, tags, nl, nc):
    '''Doubles of scratch flow_form_block_newton needs for these jobs
    (include/flow_hip.h); with 'matrix' jobs or 'vector' jobs only, what
    flow_form_block_matrix / flow_form_block_vector need: (blocks present + 1
    where a block has several programs) * nl**rank * nc.'''
    blocks = [t for k, t in zip(kinds, tags) if k != 'vector']
    comps = [t if k == 'vector' else t // 2
             for k, t in zip(kinds, tags) if k != 'matrix']
    n = len(set(blocks)) * nl * nl * nc + len(set(comps)) * nl * nc
    if len(blocks) > len(set(blocks)):
        n += nl * nl * nc
    elif len(comps) > len(set(comps)):
        n += nl * nc
    return n


def _launch_dx(mesh, lay, kind, fs, vals, vec):
    '''The dx launch of one program on a scalar space: flow_form_newton (into
    the plane `vals` and the vector `vec`), flow_form_matrix (`vals`) or
    flow_form_vector (`vec`).'''
    lib = _hip.lib()
    nl = lay.nloc
    ms, ss = ctypes.byref(mesh_struct(mesh)), ctypes.byref(space_struct(lay))
    if kind == 'newton':
        n = (nl * nl + nl) * mesh.num_cells()
        _hip.check(lib.flow_form_newton(
            ms, ss, ctypes.byref(fs), _hip.f64(scratch(mesh, n), n, 'scratch'),
            _hip.f64(vals, lay.nnz, 'vals'), _hip.f64(vec, lay.N, 'b'),
            _hip.stream()))
    elif kind == 'matrix':
        n = nl * nl * mesh.num_cells()
        _hip.check(lib.flow_form_matrix(
            ms, ss, ctypes.byref(fs), _hip.f64(scratch(mesh, n), n, 'scratch'),
            _hip.f64(vals, lay.nnz, 'vals'), _hip.stream()))
    else:
        n = nl * mesh.num_cells()
        _hip.check(lib.flow_form_vector(
            ms, ss, ctypes.byref(fs), _hip.f64(scratch(mesh, n), n, 'scratch'),
            _hip.f64(vec, lay.N, 'b'), _hip.stream()))


@functools.lru_cache(maxsize=256)
def _block_call(kinds, tags, nl, nc):
    '''(kinds, tags as C int arrays, doubles of scratch) of one block launch;
    the arrays are only read, so the calls of a held assembler share them.'''
    n = len(kinds)
    return ((ctypes.c_int * n)(*[_BLOCK_KINDS[k] for k in kinds]),
            (ctypes.c_int * n)(*tags),
            _block_newton_scratch(kinds, tags, nl, nc))


def _launch_block_dx(mesh, lay, structs, kinds, tags, vals, stride, vec):
    '''The dx launch of the programs of one call on a vector space (kinds,
    tags: tuples): flow_form_block_newton (into the four planes `vals` and
    the vector `vec` of 2N), flow_form_block_matrix (vec None) or
    flow_form_block_vector (vals None).'''
    lib = _hip.lib()
    ckinds, ctags, ns = _block_call(kinds, tags, lay.nloc, mesh.num_cells())
    ms, ss = ctypes.byref(mesh_struct(mesh)), ctypes.byref(space_struct(lay))
    buf = _hip.f64(scratch(mesh, ns), ns, 'scratch')
    if vec is None:
        _hip.check(lib.flow_form_block_matrix(
            ms, ss, len(kinds), structs, ctags, buf,
            _hip.f64(vals, 4 * stride, 'vals'), stride, _hip.stream()))
    elif vals is None:
        _hip.check(lib.flow_form_block_vector(
            ms, ss, len(kinds), structs, ctags, buf,
            _hip.f64(vec, 2 * lay.N, 'b'), _hip.stream()))
    else:
        _hip.check(lib.flow_form_block_newton(
            ms, ss, len(kinds), structs, ckinds, ctags, buf, ns,
            _hip.f64(vals, 4 * stride, 'vals'), stride,
            _hip.f64(vec, 2 * lay.N, 'b'), _hip.stream()))


def _program_structs(items, mesh):
    '''(flow_form structs of [(Program, degree, scheme, facet)] as one ctypes
    array, which the block launches take whole; keep-alives).  The structs
    hold pointers to the fields' data, which Newton updates in place.'''
    structs = (_hip.FormS * len(items))()
    keeps = []
    for k, (prog, q, scheme, facet) in enumerate(items):
        structs[k], keep = _form_struct(prog, mesh, q, facet, scheme)
        keeps.append(keep)
    return structs, keeps


def _refresh_constants(program, consts):
    '''The current values of a Program's Constants into the `consts` of its
    struct (the field's view, taken once: a held assembler keeps it);
    returns their number.'''
    values = program.constant_values()
    for i, value in enumerate(values):
        consts[i] = value
    return len(values)


class _FacetTarget(object):
    '''Where a held assembler gathers a ds or a dx(k) program: a zeroed buffer
    (N | nnz doubles) the gather writes the same entries of at every call --
    its map's targets --, zeroed again where facet_map / cell_map returns
    another tuple (the markers were changed: other targets).  `into`: where a
    further program of a block is added afterwards, else None.'''

    def __init__(self, buf, into=None):
        self.buf = buf
        self.into = into
        self.fmap = None

    def gather(self, mesh, lay, rank, fs, part):
        fmap = _selection_map(mesh, lay, rank, part)
        if self.fmap is not None and self.fmap is not fmap:
            _hip.fill(self.buf, 0.0)
        self.fmap = fmap
        _selection_arguments(mesh, lay, rank, fs, part, self.buf)
        if self.into is not None:
            axpby(1.0, self.buf, 1.0, self.into)
        return self.buf


class _Sum(object):
    '''A signed sum of contributions, added in the order given: `total` a
    held buffer, or None (the first contribution decides).  `direct`, the
    caller's rule: the first contribution may land in the total as it is, if
    its sign is +1 -- no fill, no axpby, and x stays x where 0.0 + 1.0*x would
    turn a -0.0 into 0.0.  Every other first contribution is added to zeros.
    The entry points differ in what they pass, on purpose: their bits and
    their launch counts are kept.'''

    def __init__(self, total=None):
        self.total = total
        self.first = True

    def target(self, sign, direct):
        '''The held total where the next contribution may be written straight
        into it, else None (a buffer of the caller's, then add()).'''
        return self.total if self.first and direct and sign == 1.0 else None

    def add(self, sign, out, direct=False):
        if out is not self.total:
            if self.total is None and self.first and direct and sign == 1.0:
                self.total = out
            else:
                if self.total is None:
                    self.total = device.empty(out.numel())
                if self.first:
                    _hip.fill(self.total, 0.0)
                axpby(sign, out, 1.0, self.total)
        self.first = False


class NewtonAssembler(object):
    '''(J, F) at the current values of the fields, into buffers that live as
    long as the object: a Matrix `A` (kind 0; V a vector space: kind 2) and a
    vector `b` (N; 2N), through the jobs of newton_jobs.  The structs are
    built once; the Constants' values are refreshed by every assemble().
    `fused`: _scalar_jobs_fused / block_jobs_fused of the jobs.

    Scalar space: every job is a launch, added to the total program by
    program; the first dx result of sign +1 lands in the total, any other
    goes to a spare buffer first, and a ds result is always added (to zeros
    where it is the first).  Vector space: every part of J owns four value
    planes and every part of F a vector of 2N; the dx jobs of a call are one
    launch into them, a ds part goes block by block, program by program, into
    the plane or component of its part's buffer (a further program of a block
    into a zeroed buffer of its own, then added); after all launches the
    parts are added in the order written, as assemble() adds them -- the
    total IS the first buffer only where a single dx part of sign +1 makes
    the sum.  A ds program, and a dx(k) program, owns a _FacetTarget; `route`
    is 'by_parts' where the jobs hold one, else 'fused' or 'pair' as `fused`
    tells -- 'by_parts' names that treatment (a part over a selection is
    gathered on its own into a zeroed buffer and then added), on scalar and on
    vector spaces alike, not the method _by_parts, which is the vector-space
    path.  A and b have the bits of assemble(J) and assemble(F).'''

    def __init__(self, J, F, V, form_compiler_parameters=None, fuse=True):
        self.V = V
        self.mesh = mesh = V.mesh()
        lay = V.layout
        self.parts = (J.terms(), F.terms())
        for parts in self.parts:
            for _, part in parts:
                _check_part_mesh(part, mesh)
        self.jobs = jobs = newton_jobs(J, F, form_compiler_parameters, fuse)
        # 'by_parts': a part runs over a selection (ds, dx(k)) and is gathered
        # on its own into a zeroed buffer; else what `fused` tells
        self.route = 'by_parts' if any(j.part is not None for j in jobs) \
            else None
        self._targets = {}          # per ds job: its _FacetTarget
        if V.dim == 1:
            self.fused = _scalar_jobs_fused(jobs)
            self.route = self.route or ('fused' if self.fused else 'pair')
            self.A = Matrix(lay, 0, value_plane(lay))
            self.b = device.empty(lay.N)
            self._spares = {}
            self._keep = _program_structs(
                [(j.program, j.degree, j.scheme, j.kind.startswith('facet'))
                 for j in jobs], mesh)
            self._steps = [(j, fs, fs.consts)
                           for j, fs in zip(jobs, self._keep[0])]
            return
        self.fused = block_jobs_fused(jobs)
        self.route = self.route or ('fused' if self.fused else 'pair')
        if not self.parts[0] or not self.parts[1]:
            raise ValueError('an empty sum of forms has no rank')
        # (zeroed once: the launches write the nnz entries of a plane, not
        # the one behind them)
        sizes = (4 * plane_stride(lay), 2 * lay.N)
        self._bufs = [[device.zeros(n) for _ in parts]
                      for n, parts in zip(sizes, self.parts)]
        totals = [bufs[0] if self._single_dx(parts) and parts[0][0] == 1.0
                  else device.zeros(n)
                  for n, parts, bufs in zip(sizes, self.parts, self._bufs)]
        self.A, self.b = Matrix(lay, 2, totals[0]), totals[1]
        # the launches: the jobs of a call (a part of J, of F, or a fused
        # pair) as [call, job numbers, kinds, tags, structs, keep-alives]
        self._calls = []
        for call, g in itertools.groupby(range(len(jobs)),
                                         key=lambda n: jobs[n].call):
            jns = list(g)
            js = [jobs[n] for n in jns]
            structs, keeps = _program_structs(
                [(j.program, j.degree, j.scheme, j.kind.startswith('facet'))
                 for j in js], mesh)
            self._calls.append(
                (call, jns, tuple(j.kind for j in js),
                 tuple(j.tag for j in js), structs,
                 [(j.program, fs.consts) for j, fs in zip(js, structs)],
                 keeps))

    @staticmethod
    def _single_dx(parts):
        return len(parts) == 1 and parts[0][1].integral_type == 'cell' \
            and not is_cell_subdomain(parts[0][1])

    def assemble(self):
        if self.V.dim == 2:
            self._by_parts()
        else:
            self._by_programs()
        return self.A, self.b

    def _by_programs(self):
        lay, mesh = self.V.layout, self.mesh
        msum, vsum = _Sum(self.A.vals), _Sum(self.b)
        for jn, (job, fs, consts) in enumerate(self._steps):
            _refresh_constants(job.program, consts)
            kind = job.kind
            vals = vec = None
            if job.part is not None:
                # (a ds result is never the total itself)
                rank = 2 if kind.endswith('_matrix') else 1
                target = self._targets.get(jn)
                if target is None:
                    target = self._targets[jn] = _FacetTarget(
                        value_plane(lay) if rank == 2 else device.zeros(lay.N))
                out = target.gather(mesh, lay, rank, fs, job.part)
                if rank == 2:
                    vals = out
                else:
                    vec = out
            else:
                if kind != 'vector':
                    vals = msum.target(job.msign, True)
                    if vals is None:
                        vals = self._spare(2)
                if kind != 'matrix':
                    vec = vsum.target(job.vsign, True)
                    if vec is None:
                        vec = self._spare(1)
                _launch_dx(mesh, lay, kind, fs, vals, vec)
            if vals is not None:
                msum.add(job.msign, vals)
            if vec is not None:
                vsum.add(job.vsign, vec)
        if msum.first or vsum.first:
            raise ValueError('an empty sum of forms has no rank')

    def _spare(self, rank):
        '''Where a dx result goes that cannot land in the total.'''
        buf = self._spares.get(rank)
        if buf is None:
            lay = self.V.layout
            buf = self._spares[rank] = value_plane(lay) if rank == 2 else \
                device.empty(lay.N)
        return buf

    def _by_parts(self):
        lay, mesh = self.V.layout, self.mesh
        stride = plane_stride(lay)
        for (ji, fi), jns, kinds, tags, structs, consts, _ in self._calls:
            for program, view in consts:
                _refresh_constants(program, view)
            vals = None if ji is None else self._bufs[0][ji]
            vec = None if fi is None else self._bufs[1][fi]
            if kinds[0].startswith(('facet', 'cells')):
                rank = 2 if vec is None else 1
                self._facet_blocks(jns, tags, structs, rank,
                                   vals if rank == 2 else vec)
            else:
                _launch_block_dx(mesh, lay, structs, kinds, tags, vals,
                                 stride, vec)
        for parts, bufs, total in zip(self.parts, self._bufs,
                                      (self.A.vals, self.b)):
            total = _Sum(total)
            direct = self._single_dx(parts)
            for (sign, _), buf in zip(parts, bufs):
                total.add(sign, buf, direct)

    def _facet_blocks(self, jns, tags, structs, rank, buf):
        '''The ds programs of one part into the planes or components of its
        buffer: the first program of a block straight into it, a further one
        into a zeroed buffer of its own, then added.'''
        lay = self.V.layout
        for k, jn in enumerate(jns):
            target = self._targets.get(jn)
            if target is None:
                width = lay.nnz if rank == 2 else lay.N
                step = plane_stride(lay) if rank == 2 else lay.N
                dst = buf[tags[k] * step:tags[k] * step + width]
                target = self._targets[jn] = _FacetTarget(dst) \
                    if tags[k] not in tags[:k] \
                    else _FacetTarget(device.zeros(width), dst)
            target.gather(self.mesh, lay, rank, structs[k],
                          self.jobs[jn].part)


def newton_solve(F, u, bcs=None, J=None, solver_parameters=None,
                 form_compiler_parameters=None):
    '''solve(F == 0, u, bcs, J): dolfin's NewtonSolver on the device.  F: a
    form of rank 1 in TestFunction(V) that holds the Function u of V; J: its
    Jacobian, derivative(F, u) by default.  u[dof] = g first; then, per
    iteration: (J, F) at u in one pass where the parts pair up
    (flow_form_newton; `fused` of the returned NewtonInfo tells), the
    conditions applied homogeneously (the symmetric elimination of
    assemble_system, F[dof] = 0), r = |F|_2 -- the one read-back of an
    iteration besides those of the Krylov solve --, stop where r <
    absolute_tolerance or r / r0 < relative_tolerance, else J delta = F from
    a zero start with the method and preconditioner rule of the linear solve
    (CG + Jacobi for symmetric tables or solver_parameters['symmetric'],
    else GMRES + ILU(0)) and u -= relaxation_parameter * delta.
    solver_parameters: 'nonlinear_solver' 'newton'; 'newton_solver' with
    dolfin's keys and defaults (NEWTON_DEFAULTS; 'linear_solver' and
    'krylov_solver' as for the linear solve; 'report' prints a line per
    iteration through message.info).  Raises _hip.NotConverged unless
    'error_on_nonconvergence' is False.  Not on strips.  F on a vector space
    W (forms.vector_derivatives(True)): the same loop with a kind-2 matrix and
    vectors of 2N -- (J, F) by flow_form_block_newton where rows fuse
    (newton_jobs, _block_rows), conditions on W and W.sub(i), the elimination of
    flow_bc_symmetric_blocks.'''
    from . import forms
    from ..message import info as say
    ns, symmetric = newton_parameters(solver_parameters)
    if not isinstance(F, forms.Form) or F.rank != 1:
        raise ValueError('solve(F == 0, u): F must be a form of rank 1, '
                         'linear in a test function')
    V = F.arguments()[0]
    if V.dim != 1 and not forms.vector_derivatives.enabled:
        raise NotImplementedError(
            'solve(F == 0) on a vector space: derivative() with respect to a '
            'vector Function and the Newton assembler are scalar only')
    if not isinstance(u, Function) or not u.function_space().same_as(V):
        raise ValueError('solve writes into a Function of the space of the '
                         'test function')
    if not any(forms.depends_on(p.integrand.comps, u) for _, p in F.terms()):
        raise ValueError('solve(F == 0, u): the form does not depend on u')
    if J is None:
        J = forms.derivative(F, u)
    elif not isinstance(J, forms.Form) or J.rank != 2 \
            or not J.arguments()[0].same_as(V):
        raise ValueError('J must be a bilinear form (rank 2) on the space of '
                         'u')
    symmetric = symmetric or all(
        forms.is_symmetric_table(part.argument_table()[1])
        for _, part in J.terms())
    method = ns['linear_solver']
    if method in ('default', 'iterative'):
        method = 'cg' if symmetric else 'gmres'
    asm = NewtonAssembler(J, F, V, form_compiler_parameters)
    ks = ns['krylov_solver']
    dofs, vals, mask = _scalar_bcs(bcs, V)
    if dofs is not None:
        _set_values(dofs, vals, u.data)
        zero = device.zeros(dofs.numel())
        Abc = Matrix(V.layout, 2 if V.dim == 2 else 0)
    delta = device.empty(V.size())
    ilu = None
    out = NewtonInfo(asm.fused, method, asm.route)
    rtol, atol = ns['relative_tolerance'], ns['absolute_tolerance']
    maxit = int(ns['maximum_iterations'])
    r0 = None
    while True:
        A, b = asm.assemble()
        if dofs is not None:
            A = symmetric_bc_blocks(A, mask, Abc) if V.dim == 2 else \
                symmetric_bc_matrix(A, mask, Abc)
            _set_values(dofs, zero, b)
        r = vector_norm(b)
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
        if method != 'cg' and not symmetric:
            if ilu is None:
                from .ilu import Ilu0
                ilu = Ilu0(A)
            else:
                ilu.refactor(A)
        _hip.fill(delta, 0.0)
        kinfo = krylov_solve(
            method, A, b, delta, ks.get('relative_tolerance', 1.0e-12),
            atol=ks.get('absolute_tolerance', 0.0),
            maxit=int(ks.get('maximum_iterations', 1000)), ilu=ilu,
            check_every=10, x_is_zero=True)
        out.method = kinfo.method
        out.linear_iterations.append(kinfo.iterations)
        axpby(-float(ns['relaxation_parameter']), delta, 1.0, u.data)
        out.iterations += 1
    if not out.converged and ns['error_on_nonconvergence']:
        raise _hip.NotConverged(
            'Newton solver did not converge: %d iterations, |F| = %.3e '
            '(absolute tolerance %.3e), |F| / |F0| = %.3e (relative '
            'tolerance %.3e)' % (out.iterations, r, atol, rel, rtol))
    return out


def _form_degree(form, form_compiler_parameters=None):
    from . import forms
    q = forms._quadrature_degree(form.metadata)
    if q is None:
        q = forms._quadrature_degree(form_compiler_parameters)
    return forms.check_degree(form.degree() if q is None else q)


def _interior_facet_job(form, mesh, q):
    '''(flow_form, keepalive, InteriorFacetLists) of one dS part.'''
    from . import forms
    prog = forms.compile_trees([form.integrand.comps], interior=True)
    fs, keep = _form_struct(prog, mesh, q, True)
    sel = interior_facet_lists(mesh, form.subdomain_data, form.subdomain_id)
    return fs, keep, sel


def _interior_part(form, what):
    from . import forms
    if not isinstance(form, forms.Form) or isinstance(form, forms.FormSum) \
            or form.integral_type != 'interior_facet':
        raise TypeError('%s takes one dS form, f*dS (got %r)'
                        % (what, type(form)))


def interior_facet_integrals(form, out=None, form_compiler_parameters=None):
    '''The integral of a dS form over each interior facet it selects: a
    device fp64 array with one entry per selected facet, in
    Mesh.interior_facets order (a new one, or `out`, which is returned).  One
    launch, enqueued on the package's stream: nothing synchronises.  Their
    sum is assemble(form) up to the order of the additions.'''
    _interior_part(form, 'interior_facet_integrals')
    from . import forms
    _no_strips('interior_facet_integrals')
    mesh = forms.form_mesh(form.integrand, form.mesh)
    fs, keep, sel = _interior_facet_job(
        form, mesh, _form_degree(form, form_compiler_parameters))
    if out is None:
        out = device.empty(sel.count)
    elif getattr(out, 'shape', None) != (sel.count,):
        raise ValueError('out: a device fp64 tensor of shape (%d,)'
                         % sel.count)
    if sel.count:
        _hip.check(_hip.lib().flow_form_interior_facet_values(
            ctypes.byref(mesh_struct(mesh)), ctypes.byref(fs), sel.count,
            _hip.i32(sel.plus, sel.count, 'facet + cells'),
            _hip.i32(sel.local, sel.count, 'facet + local indices'),
            _hip.i32(sel.other, sel.count, 'facet - cells'),
            _hip.f64(out, sel.count, 'out'), _hip.stream()))
    del keep
    return out


def cell_indicator(form, share=0.5, out=None, form_compiler_parameters=None):
    '''Per-cell values of a rank-0 form, or signed sum, of dx and dS parts: a
    device fp64 array (nc,) (a new one, or `out`), which feeds fem.mark
    unchanged.  A dx part gives every cell its own integral (stage 1 of the
    functional); a dx(k) part its selected cells, zeros outside the
    selection.  A dS part gives every cell `share` times the integral of
    each of its selected interior facets, added in the order of its local
    facets 0, 1, 2: 0.5 is what avg(w)*f*dS gives for a DG0 test function w,
    1.0 is Kelly's convention (JumpIndicator's).  The parts are added in the
    order written.  Enqueued; no atomics, the same bits on every call.  ds
    parts are not provided.'''
    from . import forms
    if not isinstance(form, forms.Form):
        raise TypeError('cell_indicator takes a form (got %r)' % (type(form),))
    _no_strips('cell_indicator')
    if form.rank != 0:
        raise ValueError('cell_indicator takes a form without test or trial '
                         'functions')
    lib = _hip.lib()
    share = float(share)
    total = mesh = None
    for sign, part in form.terms():
        if part.integral_type == 'exterior_facet':
            raise NotImplementedError(
                'cell_indicator of a ds part: dx and dS parts only')
        pmesh = forms.form_mesh(part.integrand, part.mesh)
        if mesh is not None and pmesh is not mesh:
            raise ValueError('the parts of the form live on different meshes')
        mesh = pmesh
        nc = mesh.num_cells()
        if total is None:
            if out is None:
                out = device.empty(nc)
            elif getattr(out, 'shape', None) != (nc,):
                raise ValueError('out: a device fp64 tensor of shape (%d,)'
                                 % nc)
        # (a first part of sign +1 lands in `out` itself, the others in a
        # spare that is added to it)
        direct = total is None and sign == 1.0
        dest = out if direct else device.empty(nc)
        if part.integral_type == 'interior_facet':
            sel = interior_facet_lists(mesh, part.subdomain_data,
                                       part.subdomain_id)
            vals = interior_facet_integrals(
                part, form_compiler_parameters=form_compiler_parameters)
            if sel.count == 0:
                _hip.fill(dest, 0.0)
            else:
                _hip.check(lib.flow_facet_cell_shares(
                    ctypes.byref(mesh_struct(mesh)), sel.count,
                    _hip.i32(sel.cell_positions, 3 * nc, 'cell positions'),
                    _hip.f64(vals, sel.count, 'facet integrals'), share,
                    _hip.f64(dest, nc, 'out'), _hip.stream()))
        else:
            q = _form_degree(part, form_compiler_parameters)
            prog = forms.compile_trees([part.integrand.comps])
            fs, keep = _form_struct(prog, mesh, q)
            if is_cell_subdomain(part):
                # (zeros outside the selection: the launch writes its cells)
                cells, nsel = cell_lists(mesh, part.subdomain_data,
                                         part.subdomain_id)
                _hip.fill(dest, 0.0)
                if nsel:
                    _hip.check(lib.flow_form_cells_values(
                        ctypes.byref(mesh_struct(mesh)), ctypes.byref(fs),
                        nsel, _hip.i32(cells, nsel, 'cell list'),
                        _hip.f64(dest, nc, 'out'), _hip.stream()))
            else:
                _hip.check(lib.flow_form_cell_values(
                    ctypes.byref(mesh_struct(mesh)), ctypes.byref(fs),
                    _hip.f64(dest, nc, 'out'), _hip.stream()))
            del keep
        if not direct:
            if total is None:
                _hip.fill(out, 0.0)
            axpby(sign, dest, 1.0, out)
        total = out
    if total is None:
        raise ValueError('cell_indicator: the form has no parts')
    return out


def _list_launch(fn, head, mesh, lists, count, lmap, per_item, out, tail=()):
    '''The element launch over a list and the gather launch, one C call `fn`
    of the shape (*head, count, *lists, nt, targets, ptr, src, scratch, out,
    *tail, stream).  head: the mesh, space and form structs by reference;
    lists: [(device int32 array of `count` entries, its label)] -- the cells,
    or the cells and the local facet indices; lmap: the contribution map
    (targets, ptr, src, nt) of the list; per_item: element entries per item
    of the list; out: (buffer, its length, its label), written at the map's
    targets only.  An empty list launches nothing.'''
    if count == 0:
        return
    targets, ptr, src, nt = lmap
    n = per_item * count
    buf, length, label = out
    _hip.check(fn(
        *head, count, *[_hip.i32(a, count, what) for a, what in lists], nt,
        _hip.i32(targets, nt, 'map targets'), _hip.i32(ptr, nt + 1, 'map ptr'),
        _hip.i32(src, n, 'map src'), _hip.f64(scratch(mesh, n), n, 'scratch'),
        _hip.f64(buf, length, label), *tail, _hip.stream()))


def _selection_lists(mesh, part):
    '''(lists, count) of a ds or dx(k) part as _list_launch takes them:
    facet_lists | cell_lists with the labels of their arrays.'''
    if part.integral_type == 'cell':
        cells, nsel = cell_lists(mesh, part.subdomain_data, part.subdomain_id)
        return [(cells, 'cell list')], nsel
    cells, local, nf = facet_lists(mesh, part.subdomain_data,
                                   part.subdomain_id)
    return [(cells, 'facet cells'), (local, 'facet local indices')], nf


def _selection_map(mesh, lay, rank, part):
    '''The contribution map of a ds or dx(k) part.'''
    fn = cell_map if part.integral_type == 'cell' else facet_map
    return fn(mesh, lay, rank, part.subdomain_data, part.subdomain_id)


def _selection_arguments(mesh, lay, rank, fs, part, out):
    '''One ds or dx(k) part of rank 1 | 2 into `out` (N | nnz doubles, zero
    outside the map's targets): flow_form_facet_matrix / _vector over the
    facet lists, flow_form_cells_matrix / _vector over the cell list.'''
    lib = _hip.lib()
    if part.integral_type == 'cell':
        fn = lib.flow_form_cells_matrix if rank == 2 \
            else lib.flow_form_cells_vector
    else:
        fn = lib.flow_form_facet_matrix if rank == 2 \
            else lib.flow_form_facet_vector
    _list_launch(
        fn, (ctypes.byref(mesh_struct(mesh)), ctypes.byref(space_struct(lay)),
             ctypes.byref(fs)), mesh, *_selection_lists(mesh, part),
        _selection_map(mesh, lay, rank, part), lay.nloc**rank,
        (out, lay.nnz if rank == 2 else lay.N, 'out'))


def form_load_vector(expr, V, form_compiler_parameters=None):
    '''b_(a,i) = int expr_a phi_i over the test functions of V: the load
    vector of project(expr, V).'''
    from . import forms
    if expr.shape != (() if V.dim == 1 else (V.dim,)):
        raise ValueError('projecting an expression of shape %r into a space '
                         'with %d components' % (expr.shape, V.dim))
    forms.check_no_normal(expr, 'project')
    _no_strips('project of an expression')
    lib = _hip.lib()
    mesh = forms.form_mesh(expr, V.mesh())
    q = forms.projection_degree(expr, V.degree, form_compiler_parameters)
    prog = forms.compile_trees(expr.scalar_trees())
    fs, keep = _form_struct(prog, mesh, q)
    lay = V.layout
    b = device.empty(V.size())
    buf = scratch(mesh, V.dim * lay.nloc * mesh.num_cells())
    _hip.check(lib.flow_form_load_vector(
        ctypes.byref(mesh_struct(mesh)), ctypes.byref(space_struct(lay)),
        ctypes.byref(fs), _hip.f64(buf), _hip.f64(b), _hip.stream()
        ))
    del keep
    return b
