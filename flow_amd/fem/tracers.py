# -*- coding: utf-8 -*-
'''
Lagrangian tracer particles: a `Probes` whose points move with a velocity
field, dx/dt = u(x, t), integrated on the GPU (flow_advect_points,
csrc/form_kernels.hip: advect_points_kernel).

State, on the device, in the layout of flow_locate_points / flow_form_points:
positions SoA (2, n) fp64, owning cell (n,) int32 (-1: lost), barycentric
coordinates (3, n).  After every call the cell and the barycentrics of a live
particle are what flow_locate_points returns for its position (the
lowest-index rule of flow_amd/fem/points.py).

Loss rule: a substep is accepted if every point at which it evaluates the
velocity, and its end point, lies in some cell by the tolerance of the
location test (min lambda >= -1e-12).  Otherwise the particle is lost: its
position stays what it was at the start of that substep, its cell becomes -1,
and every later substep and call leaves it alone.  Particles leave through the
outflow or numerically enter the obstacle; that is normal.

Not on strips.
'''
import math

import numpy

from .points import as_points, _grid_struct

# flow_advect_points: scheme (include/flow_hip.h, FLOW_ADVECT_*)
SCHEMES = {'euler': 1, 'rk2': 2, 'rk4': 4}


def _velocity_space(u, what='u'):
    V = u.function_space() if hasattr(u, 'function_space') else None
    if V is None or not hasattr(V, 'layout') or getattr(V, 'dim', 0) != 2 \
            or getattr(V, 'component', None) is not None:
        raise ValueError('%s: a Function on a VectorFunctionSpace(mesh, '
                         "'CG', 1 or 2), not a scalar, component or mixed "
                         'space' % what)
    if V.degree not in (1, 2):
        raise ValueError('%s: degree %r, tracers follow P1 and P2 fields'
                         % (what, V.degree))
    return V


class Tracers(object):
    '''Particles that follow a velocity field.

        tracers = Tracers(mesh, seeds)
        tracers.advect(u, dt, steps=10)             # frozen field, RK4
        tracers.advect(u0, dt, u_next=u1)           # linear in time
        tracers.positions(), tracers.alive()
        tracers(p)                                  # a field at the particles

    A point in no cell starts lost (cell -1).'''

    def __init__(self, mesh, points):
        import torch
        from .. import device
        from .ops import _no_strips
        _no_strips('Tracer particles')
        self.mesh = mesh
        dev = device.get()
        self.n = 0
        self._xy = torch.empty((2, 0), dtype=torch.float64, device=dev)
        self._cell = torch.empty((0,), dtype=torch.int32, device=dev)
        self._bary = torch.empty((3, 0), dtype=torch.float64, device=dev)
        self.inject(points)

    def __len__(self):
        return self.n

    # -- the particles ----------------------------------------------------------
    def inject(self, points):
        '''Append new particles and locate them; the particles held keep
        their indices.'''
        import ctypes
        import torch
        from .. import _hip, device
        from .ops import _no_strips, mesh_struct
        _no_strips('Tracer particles')
        pts = as_points(points)
        m = len(pts)
        if not m:
            return
        xy = device.to_device(pts.T.copy())
        cell = torch.empty(m, dtype=torch.int32, device=xy.device)
        bary = device.empty(3 * m)
        _hip.check(_hip.lib().flow_locate_points(
            ctypes.byref(mesh_struct(self.mesh)),
            ctypes.byref(_grid_struct(self.mesh)), m,
            _hip.f64(xy, 2 * m, 'points'), _hip.i32(cell, m, 'cells'),
            _hip.f64(bary, 3 * m, 'barycentric coordinates'), _hip.stream()))
        self._xy = torch.cat([self._xy, xy], dim=1).contiguous()
        self._cell = torch.cat([self._cell, cell]).contiguous()
        self._bary = torch.cat([self._bary, bary[:3 * m].view(3, m)],
                               dim=1).contiguous()
        self.n += m

    def compact(self):
        '''Drop the lost particles, keeping the order of the others; the
        indices kept, numpy int64.'''
        import torch
        from .. import device
        device.synchronize()
        keep = torch.nonzero(self._cell >= 0).reshape(-1)
        self._xy = self._xy[:, keep].contiguous()
        self._cell = self._cell[keep].contiguous()
        self._bary = self._bary[:, keep].contiguous()
        self.n = int(keep.numel())
        return keep.cpu().numpy()

    def positions(self):
        from .. import device
        return device.to_host(self._xy).numpy().T.copy()

    def cells(self):
        from .. import device
        return device.to_host(self._cell).numpy().copy()

    def alive(self):
        return self.cells() >= 0

    # -- motion -----------------------------------------------------------------
    def advect(self, u, dt, steps=1, scheme='rk4', u_next=None):
        '''`steps` substeps of size dt (negative: backwards) of 'euler',
        'rk2' (midpoint) or 'rk4' (classical) in one kernel launch, no
        read-back.  Without u_next the field is frozen; with it the velocity
        at fraction theta of the call's time steps * dt is (1 - theta) u +
        theta u_next, at each stage's own time.'''
        import ctypes
        from .. import _hip
        from .ops import _no_strips, mesh_struct, space_struct
        _no_strips('Tracer particles')
        V = _velocity_space(u)
        if V.mesh() is not self.mesh:
            raise ValueError('u lives on another mesh than the tracers')
        if u_next is not None:
            Vn = _velocity_space(u_next, 'u_next')
            if not V.same_as(Vn):
                raise ValueError('u_next: not a Function of the space of u')
        if scheme not in SCHEMES:
            raise ValueError("scheme %r: 'euler', 'rk2' or 'rk4'" % (scheme,))
        if isinstance(steps, bool) or int(steps) != steps or steps < 1:
            raise ValueError('steps: a positive integer, got %r' % (steps,))
        dt = float(dt)
        if not math.isfinite(dt):
            raise ValueError('dt: a finite number, got %r' % (dt,))
        n = self.n
        if not n:
            return
        lay = V.layout
        _hip.check(_hip.lib().flow_advect_points(
            ctypes.byref(mesh_struct(self.mesh)),
            ctypes.byref(_grid_struct(self.mesh)),
            ctypes.byref(space_struct(lay)),
            _hip.f64(u.data, 2 * lay.N, 'u'),
            None if u_next is None else _hip.f64(u_next.data, 2 * lay.N, 'u_next'),
            n, _hip.f64(self._xy, 2 * n, 'points'),
            _hip.i32(self._cell, n, 'cells'),
            _hip.f64(self._bary, 3 * n, 'barycentric coordinates'),
            dt, int(steps), SCHEMES[scheme], _hip.stream()))

    # -- fields at the particles ------------------------------------------------
    def evaluate(self, f, out=None):
        '''f at the particles as a device fp64 tensor (value_size, n), NaN
        for lost particles: Probes.evaluate at the moving points.'''
        import ctypes
        from .. import _hip, device
        from . import forms
        from .ops import _form_struct, _no_strips, mesh_struct
        _no_strips('Tracer particles')
        expr = forms.as_form(f)
        forms._join_mesh(expr.mesh, self.mesh)
        prog = forms.point_program(expr)
        nout, n = prog.nout, self.n
        if out is None:
            out = device.empty(max(nout * n, 1))[:nout * n].view(nout, n)
        elif tuple(out.shape) != (nout, n):
            raise ValueError('out: shape %r, the values have shape %r'
                             % (tuple(out.shape), (nout, n)))
        if n:
            fs, keep = _form_struct(prog, self.mesh, 0)
            _hip.check(_hip.lib().flow_form_points(
                ctypes.byref(mesh_struct(self.mesh)), ctypes.byref(fs), n,
                _hip.i32(self._cell, n, 'cells'),
                _hip.f64(self._bary, 3 * n, 'barycentric coordinates'),
                _hip.f64(out, nout * n, 'out'), _hip.stream()))
            del keep
        return out

    def __call__(self, f):
        '''f at the particles, on the host: (n,) for a scalar, (n, 2) for a
        vector; NaN for lost particles.'''
        from .. import device
        vals = device.to_host(self.evaluate(f)).numpy()
        return vals[0].copy() if vals.shape[0] == 1 else vals.T.copy()
