# -*- coding: utf-8 -*-
'''
Cost of tracer particles ("Tracer particles"): 1 M
particles seeded uniformly over the bench mesh KarmanProblem(2182, 509), its
P2 velocity after a few IPCS steps, RK4, 10 substeps.

  fused     flow_advect_points: one launch for all substeps;
  composed  the same trajectory from what the library had before it: per
            stage one flow_locate_points and one flow_form_points of the
            velocity, and the torch updates of the stage points, the
            accumulators and the loss mask, driven from Python (four pairs
            per RK4 substep).

HIP events, 2 warm-up calls, median of 7 with min and max; every call starts
from the same seeded state (restored outside the timed region).  Prints the
time per particle-substep of both, the share of lost particles, and the
largest distance between the two end states.

    python tools/tracer_lab.py [nx [ny]] [--particles N] [--steps K] [--ns-steps M]
'''
import ctypes
import os
import sys

import numpy
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from flow_amd import fem, device, karman, _hip       # noqa: E402
from flow_amd.fem import forms                       # noqa: E402
from flow_amd.fem.ops import _form_struct, mesh_struct   # noqa: E402
from flow_amd.fem.points import _grid_struct         # noqa: E402


def timed(call, reset, warmup=2, repeat=7):
    for _ in range(warmup):
        reset()
        call()
    device.synchronize()
    ms = []
    for _ in range(repeat):
        reset()
        device.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), \
            torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return numpy.median(ms), min(ms), max(ms)


class Composed(object):
    '''RK4 from flow_locate_points + flow_form_points + torch.'''

    def __init__(self, mesh, u, xy, cell):
        self.mesh, self.n = mesh, xy.shape[1]
        n = self.n
        self.xy, self.cell = xy, cell
        self.alive = torch.empty(n, dtype=torch.bool, device=xy.device)
        self.ok = torch.empty_like(self.alive)
        self.sp = torch.empty_like(xy)
        self.sc = torch.empty_like(cell)
        self.sb = device.empty(3 * n)
        self.k = [device.empty(2 * n).view(2, n) for _ in range(4)]
        prog = forms.point_program(forms.as_form(u))
        self.fs, self.keep = _form_struct(prog, mesh, 0)
        self.lib = _hip.lib()
        self.ms, self.gs = mesh_struct(mesh), _grid_struct(mesh)

    def velocity(self, pts, out):
        '''cells of pts and the velocity there; ok &= found'''
        n = self.n
        _hip.check(self.lib.flow_locate_points(
            ctypes.byref(self.ms), ctypes.byref(self.gs), n,
            _hip.f64(pts, 2 * n), _hip.i32(self.sc, n), _hip.f64(self.sb, 3 * n),
            _hip.stream()))
        _hip.check(self.lib.flow_form_points(
            ctypes.byref(self.ms), ctypes.byref(self.fs), n, _hip.i32(self.sc, n),
            _hip.f64(self.sb, 3 * n), _hip.f64(out, 2 * n), _hip.stream()))
        self.ok &= self.sc >= 0
        # (the lanes that are lost carry NaN: keep them finite for the sums)
        torch.nan_to_num_(out, nan=0.0)

    def advect(self, dt, steps):
        k1, k2, k3, k4 = self.k
        torch.ge(self.cell, 0, out=self.alive)
        for _ in range(steps):
            self.ok.copy_(self.alive)
            self.velocity(self.xy, k1)
            torch.add(self.xy, k1, alpha=0.5 * dt, out=self.sp)
            self.velocity(self.sp, k2)
            torch.add(self.xy, k2, alpha=0.5 * dt, out=self.sp)
            self.velocity(self.sp, k3)
            torch.add(self.xy, k3, alpha=dt, out=self.sp)
            self.velocity(self.sp, k4)
            k1.add_(k4).add_(k2, alpha=2.0).add_(k3, alpha=2.0)
            torch.add(self.xy, k1, alpha=dt / 6.0, out=self.sp)
            # the end point's cell decides with the next substep's first
            # location (here: one more, so that both paths end alike)
            _hip.check(self.lib.flow_locate_points(
                ctypes.byref(self.ms), ctypes.byref(self.gs), self.n,
                _hip.f64(self.sp, 2 * self.n), _hip.i32(self.sc, self.n),
                _hip.f64(self.sb, 3 * self.n), _hip.stream()))
            self.ok &= self.sc >= 0
            torch.where(self.ok, self.sp, self.xy, out=self.xy)
            self.alive &= self.ok
        self.cell.masked_fill_(~self.alive, -1)


def main():
    args = sys.argv[1:]

    def opt(name, default):
        if name in args:
            i = args.index(name)
            v = int(args[i + 1])
            del args[i:i + 2]
            return v
        return default

    n = opt('--particles', 1000000)
    steps = opt('--steps', 10)
    ns_steps = opt('--ns-steps', 3)
    nx = int(args[0]) if args else 2182
    ny = int(args[1]) if len(args) > 1 else int(round(nx * 509.0 / 2182.0))
    prob = karman.KarmanProblem(nx, ny)
    for _ in range(ns_steps):
        prob.step()
    mesh, u = prob.mesh, prob.u0
    umax = float(numpy.abs(u.array()).max())
    lo, hi = mesh.points.min(axis=0), mesh.points.max(axis=0)
    h = numpy.sqrt(2.0 * (hi - lo).prod() / mesh.num_cells())
    dt = 0.5 * h / max(umax, 1e-300)       # half a cell per substep at most
    print('mesh %d x %d: %d cells, P%d velocity after %d steps, max |u_i| %.3g; '
          '%d particles, rk4, %d substeps of dt %.3e'
          % (nx, ny, mesh.num_cells(), u.function_space().degree, ns_steps, umax,
             n, steps, dt))
    rng = numpy.random.RandomState(0)
    seeds = lo + rng.uniform(size=(n, 2)) * (hi - lo)
    tr = fem.Tracers(mesh, seeds)
    xy0, cell0, bary0 = tr._xy.clone(), tr._cell.clone(), tr._bary.clone()
    print('in no cell at the start: %.3f %%' % (100.0 * (~tr.alive()).mean()))

    def reset():
        tr._xy.copy_(xy0)
        tr._cell.copy_(cell0)
        tr._bary.copy_(bary0)

    fused = timed(lambda: tr.advect(u, dt, steps=steps), reset)
    end, end_cells = tr.positions(), tr.cells()
    comp = Composed(mesh, u, xy0.clone(), cell0.clone())

    def reset_c():
        comp.xy.copy_(xy0)
        comp.cell.copy_(cell0)

    composed = timed(lambda: comp.advect(dt, steps), reset_c)
    cend = device.to_host(comp.xy).numpy().T
    ccell = device.to_host(comp.cell).numpy()
    for name, (med, a, b) in (('flow_advect_points', fused),
                              ('composed', composed)):
        print('%-20s %9.3f ms (%.3f - %.3f)   %.4f ns / particle-substep'
              % (name, med, a, b, 1e6 * med / (n * steps)))
    print('composed / fused: %.2f' % (composed[0] / fused[0]))
    print('lost after the call: %.3f %% (composed path %.3f %%), lost flags '
          'that differ: %d, max |position difference| %.2e'
          % (100.0 * (end_cells < 0).mean(), 100.0 * (ccell < 0).mean(),
             ((end_cells < 0) != (ccell < 0)).sum(),
             numpy.abs(end - cend)[(end_cells >= 0) & (ccell >= 0)].max()))


if __name__ == '__main__':
    main()
