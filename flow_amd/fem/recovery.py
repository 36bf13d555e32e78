# -*- coding: utf-8 -*-
'''
Recovered nodal gradients and the Zienkiewicz-Zhu error indicator: a
derivative of a discrete field as a nodal field without a mass solve, and the
estimate of the H1-seminorm error that goes with it.

    R = GradientRecovery(V)         # V: scalar or 2-vector P1 / P2
    G = R.apply(u)                  # scalar u: a Function on
                                    # VectorFunctionSpace(mesh, 'CG', V.degree)
    G0, G1 = R.apply(u)             # 2-vector u: the rows grad(u)[0, :] and
                                    # grad(u)[1, :], each such a Function
    R.apply(u, out=G)               # into existing Function(s); returned
    eta2 = R.indicator(u)           # device fp64 (nc,): two launches, no sync
    cells = mark(eta2, 0.5)         # as with JumpIndicator
    R.estimate(u)                   # sqrt(sum eta2), a float (synchronises)

Recovery (flow_recover_gradient, csrc/recovery_kernels.hip): at every node n
of the scalar layout of V

    G_k(n) = sum_c |T_c| grad u_k|_c(x_n) / sum_c |T_c|,

the sum over the cells of the node's patch, each cell's gradient taken AT the
node (a vertex or an edge mid point of that cell), in the order of the
space's vector contribution map (layout.vmap: ascending local node, then
ascending cell): one lane per node, every component in one launch, the same
bits on every call.  Nodes on the boundary get the mean over their one-sided
patch; there is no special treatment.

Indicator (flow_zz_indicator): eta2[T] = sum_k int_T |G_k - grad u_k|^2 dx
with G_k interpolated in P_deg, one lane per cell, by triangle_rule(2 * deg)
(exact: the integrand has that degree).

The results are ordinary Functions: Probes, Tracers, forms, XDMFFile and
Transfer take them as they are.  Not on strips.
'''
import math


def _rule_dev(degree):
    '''reference.triangle_rule(2 * degree) as device rows (xi, eta, w).'''
    import numpy
    from . import reference
    from .. import device
    key = (degree, str(device.get()))
    held = _RULES.get(key)
    if held is None:
        pts, wts = reference.triangle_rule(2 * degree)
        rule = numpy.concatenate([pts, wts[:, None]], axis=1)
        held = _RULES[key] = (device.to_device(rule.reshape(-1)), len(wts))
    return held


_RULES = {}


class GradientRecovery(object):
    '''The patch-averaged gradient of Functions of V (scalar or 2-vector P1 /
    P2) and the ZZ indicator built on it; see the module's text.'''

    def __init__(self, V):
        from .ops import _no_strips
        from .space import VectorFunctionSpace
        if not hasattr(V, 'layout'):
            raise NotImplementedError(
                'V: a mixed space; recover the gradients of its sub-spaces '
                'one by one')
        if getattr(V, 'component', None) is not None:
            raise NotImplementedError(
                'V: a component view (W.sub(i)); recover the gradient of the '
                'vector field, or of a Function on W.sub(i).collapse()')
        if V.degree not in (1, 2):
            raise ValueError('V: P%r; gradient recovery takes P1 or P2'
                             % (V.degree,))
        if V.dim not in (1, 2):
            raise ValueError('V: %r components; scalar or 2-vector' % (V.dim,))
        _no_strips('Gradient recovery')
        self.V = V
        self.nc = V.mesh().num_cells()
        # the space of a recovered gradient (of one component)
        self.G = VectorFunctionSpace(V.mesh(), 'CG', V.degree)
        V.layout.vmap('vptr')
        self._work = None

    # -- operands ---------------------------------------------------------------
    def _check_u(self, u):
        from .function import Function
        if not isinstance(u, Function) \
                or not u.function_space().same_as(self.V):
            raise ValueError('u: not a Function of the space this recovery '
                             'was built for')

    def _check_out(self, out):
        '''The Functions of `out` as a list, one per component of V.'''
        from .function import Function
        fs = [out] if self.V.dim == 1 else out
        if self.V.dim == 2 and (not isinstance(out, (tuple, list))
                                or len(out) != 2):
            raise ValueError('out: a pair of Functions (G0, G1) for a '
                             '2-vector field')
        for f in fs:
            if not isinstance(f, Function) or getattr(
                    f.function_space(), 'component', None) is not None \
                    or not f.function_space().same_as(self.G):
                raise ValueError(
                    'out: not Function(s) on VectorFunctionSpace(mesh, '
                    "'CG', %d) of this mesh" % self.V.degree)
        if len(fs) == 2 and fs[0] is fs[1]:
            raise ValueError('out: the same Function twice')
        return fs

    def _launch(self, u, buf):
        '''G of u into buf (a tensor of 2 * dim * N doubles, or the checked
        address of as many), one launch.'''
        import ctypes
        from .. import _hip
        from .ops import mesh_struct, space_struct
        V = self.V
        ptr = buf if isinstance(buf, ctypes.c_void_p) else \
            _hip.f64(buf, 2 * V.dim * V.N, 'recovered gradient')
        _hip.check(_hip.lib().flow_recover_gradient(
            ctypes.byref(mesh_struct(V.mesh())),
            ctypes.byref(space_struct(V.layout)), V.dim,
            _hip.f64(u.data, V.dim * V.N, 'u'), ptr, _hip.stream()))
        return buf

    def _scratch(self):
        from .. import device
        if self._work is None:
            self._work = device.empty(2 * self.V.dim * self.V.N)
        return self._work

    # -- the recovered gradient ---------------------------------------------------
    def apply(self, u, out=None):
        '''G(u): for a scalar u a new Function on VectorFunctionSpace(mesh,
        'CG', degree); for a 2-vector u the pair (G0, G1) of such Functions,
        the gradients of the two components (new ones share one buffer).
        out: the Function, or the pair, to write into; it is returned.  One
        kernel launch on the package's stream for all components -- for a
        pair `out` whose Functions do not lie next to each other in memory
        (those a call without `out` returned do), into a buffer of this
        object, followed by one copy each.'''
        from .. import _hip, device
        from .function import Function
        from .ops import _no_strips
        _no_strips('Gradient recovery')
        self._check_u(u)
        dim, n2 = self.V.dim, 2 * self.V.N
        if out is None:
            _hip.lib()
            buf = device.empty(dim * n2)
            self._launch(u, buf)
            fs = [Function(self.G, buf[a * n2:(a + 1) * n2]) for a in range(dim)]
            return fs[0] if dim == 1 else tuple(fs)
        fs = self._check_out(out)
        _hip.lib()
        ptrs = [_hip.f64(f.data, n2, 'out') for f in fs]
        if dim == 1 or ptrs[1].value == ptrs[0].value + 8 * n2:
            # G1 right behind G0: what apply() itself hands out
            self._launch(u, ptrs[0])
        else:
            buf = self._launch(u, self._scratch())
            for a in range(2):
                _hip.copy(fs[a].data, buf[a * n2:(a + 1) * n2])
        return out

    # -- the indicator ---------------------------------------------------------
    def indicator(self, u, out=None):
        '''eta2 of the Function u on V: a new device tensor (nc,), or `out`
        (a contiguous device fp64 tensor of nc entries), which is returned.
        Two kernel launches on the package's stream (the recovery into a
        buffer of this object, then the cell integrals), no host
        synchronisation.'''
        import ctypes
        from .. import _hip, device
        from .ops import _no_strips, mesh_struct, space_struct
        _no_strips('The ZZ indicator')
        self._check_u(u)
        lib = _hip.lib()
        nc, V = self.nc, self.V
        if out is None:
            out = device.empty(nc)
        elif getattr(out, 'shape', None) != (nc,):
            raise ValueError('out: a device fp64 tensor of shape (%d,)' % nc)
        G = self._launch(u, self._scratch())
        rule, nq = _rule_dev(V.degree)
        _hip.check(lib.flow_zz_indicator(
            ctypes.byref(mesh_struct(V.mesh())),
            ctypes.byref(space_struct(V.layout)), V.dim,
            _hip.f64(u.data, V.dim * V.N, 'u'),
            _hip.f64(G, 2 * V.dim * V.N, 'recovered gradient'), nq,
            _hip.f64(rule, 3 * nq, 'quadrature rule'),
            _hip.f64(out, nc, 'eta2'), _hip.stream()))
        return out

    def estimate(self, u):
        '''sqrt(sum eta2): the estimate of |grad(u - u_exact)|_L2 on the
        whole mesh, a float.'''
        from .. import device
        total = self.indicator(u).sum()
        return math.sqrt(float(device.to_host(total)))


def recover_gradient(u):
    '''GradientRecovery(u.function_space()).apply(u), for a single use.'''
    return GradientRecovery(u.function_space()).apply(u)


def zz_indicator(u):
    '''GradientRecovery(u.function_space()).indicator(u), for a single use.'''
    return GradientRecovery(u.function_space()).indicator(u)
