# -*- coding: utf-8 -*-
'''
The adaptive loop ("Adaptive refinement"): what its
phases cost and what it buys.

  poisson   -laplace u = f on the unit square, P1, a Gaussian bump of width
            sigma as the solution: cycles of solve(a == L) -> JumpIndicator
            -> mark(fraction, 'dorfler') -> refine -> Transfer (the start
            vector of the next solve), from UnitSquareMesh(n, n).  Per cycle:
            dofs, L2 error, estimate, and the time of each phase -- the
            indicator launch (HIP events, median of 7), mark, refine and the
            Transfer's construction and apply (wall clock: they synchronise
            or run on the host);
  karman    a few IPCS steps on karman_channel(nx, fitted=True), the
            indicator of the velocity, refine, Transfer of u and p with
            allow_extrapolation=True (prints max_distance), and a few IPCS
            steps on the new mesh from the transferred state.

    python tools/adapt_lab.py [poisson|karman|all] [n] [--cycles K]
                              [--fraction F] [--sigma S]
'''
import os
import sys
import time

import numpy
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from flow_amd import fem, device       # noqa: E402
from flow_amd.fem import (              # noqa: E402
    JumpIndicator, Transfer, mark, refine, TestFunction, TrialFunction, dx,
    grad, inner,
    )


def timed(call, warmup=2, repeat=7):
    for _ in range(warmup):
        call()
    device.synchronize()
    ms = []
    for _ in range(repeat):
        a, b = torch.cuda.Event(enable_timing=True), \
            torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return numpy.median(ms), min(ms), max(ms)


def wall(call):
    device.synchronize()
    t0 = time.perf_counter()
    out = call()
    device.synchronize()
    return out, 1e3 * (time.perf_counter() - t0)


def poisson(n, cycles, fraction, sigma):
    r2 = '(pow(x[0] - 0.5, 2) + pow(x[1] - 0.5, 2))'
    ucode = 'exp(-%s / %r)' % (r2, 2.0 * sigma**2)
    fcode = '(%r - %s / %r) * %s' % (2.0 / sigma**2, r2, sigma**4, ucode)
    exact = fem.Expression(ucode, degree=5)
    mesh = fem.UnitSquareMesh(n, n)
    previous = None
    print('cycle     cells      dofs   L2 error   estimate | solve ms | '
          'indicator ms (min - max) |  mark ms | refine ms | transfer: '
          'build ms, apply ms')
    for cycle in range(cycles + 1):
        V = fem.FunctionSpace(mesh, 'CG', 1)
        u, v = TrialFunction(V), TestFunction(V)
        a = inner(grad(u), grad(v)) * dx
        L = fem.Expression(fcode, degree=4) * v * dx
        bcs = [fem.DirichletBC(V, fem.Expression(ucode, degree=4), 'on_boundary')]
        uh = fem.Function(V)
        build = apply = float('nan')
        if previous is not None:
            T, build = wall(lambda: Transfer(previous.function_space(), V))
            _, apply = wall(lambda: T.apply(previous, out=uh))
        _, solve = wall(lambda: fem.solve(a == L, uh, bcs, solver_parameters={
            'krylov_solver': {'relative_tolerance': 1e-10}}))
        J = JumpIndicator(V)
        eta2 = J.apply(uh)                   # (uploads the facet table)
        ind = timed(lambda: J.apply(uh, out=eta2))
        est = J.estimate(uh)
        cells, tm = wall(lambda: mark(eta2, fraction, 'dorfler'))
        fine, tr = wall(lambda: refine(mesh, cells))
        print('%5d %9d %9d  %.3e  %.3e | %8.2f | %8.4f (%.4f - %.4f) | %8.2f | '
              '%9.2f | %8.2f, %6.3f'
              % (cycle, mesh.num_cells(), V.N, fem.errornorm(exact, uh), est,
                 solve, ind[0], ind[1], ind[2], tm, tr, build, apply),
              flush=True)
        previous, mesh = uh, fine


def karman(nx, steps=5):
    from flow_amd import karman as kar
    prob = kar.KarmanProblem(nx, scheme='ipcs')
    prob.reset(1.0e-5)
    prob.set_initial_stokes()
    for _ in range(steps):
        prob.step()
    mesh = prob.mesh
    J = JumpIndicator(prob.W)
    eta2 = J.apply(prob.u0)
    ind = timed(lambda: J.apply(prob.u0, out=eta2))
    print('karman_channel(%d): %d cells, %d velocity dofs; indicator %.4f ms '
          '(%.4f - %.4f), estimate %.3e'
          % ((nx, mesh.num_cells(), prob.W.size()) + ind + (J.estimate(prob.u0),)))
    cells, tm = wall(lambda: mark(eta2, 0.5, 'dorfler'))
    fine, tr = wall(lambda: refine(mesh, cells))
    print('mark %.2f ms (%d cells), refine %.2f ms -> %d cells, hmin %.2e -> %.2e'
          % (tm, cells.sum(), tr, fine.num_cells(), mesh.hmin(), fine.hmin()))
    new = kar.KarmanProblem(mesh=fine, scheme='ipcs')
    new.reset(prob.dt)
    for name, src, dst in (('u', prob.u0, new.u0), ('p', prob.p0, new.p0)):
        T, build = wall(lambda: Transfer(src.function_space(), dst.function_space(),
                                         allow_extrapolation=True))
        _, apply = wall(lambda: T.apply(src, out=dst))
        print('transfer %s: build %.2f ms, apply %.3f ms; %d of %d nodes outside, '
              'max_distance %.3e'
              % (name, build, apply, (~T.found).sum(), T.n, T.distance.max()))
    new.t = prob.t
    for k in range(steps):
        new.step()
        print('step %d on the refined mesh: t %.4e dt %.3e max |u| %.4f'
              % (k, new.t, new.dt, float(new.u0.data.abs().max())), flush=True)


def main():
    args = sys.argv[1:]
    opts = {'--cycles': 8, '--fraction': 0.5, '--sigma': 0.05}
    for key in list(opts):
        if key in args:
            i = args.index(key)
            opts[key] = type(opts[key])(args[i + 1])
            del args[i:i + 2]
    what = args[0] if args else 'all'
    if what in ('poisson', 'all'):
        poisson(int(args[1]) if len(args) > 1 else 64, opts['--cycles'],
                opts['--fraction'], opts['--sigma'])
    if what in ('karman', 'all'):
        karman(int(args[1]) if len(args) > 1 and what == 'karman' else 240)


if __name__ == '__main__':
    main()
