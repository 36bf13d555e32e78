# -*- coding: utf-8 -*-
'''
Wall distributions on the cylinder ("Wall
distributions"): fem.BoundaryProfile on a Karman state.

On the mesh of KarmanProblem(nx, ny) (default 2182 x 509), from the Stokes
start and `--steps` time steps behind it, along the obstacle's curve started
at the front stagnation side (start = the point of the circle facing the
inflow):

  Cp(theta)      pressure_coefficient(p, p at the first sample, rho, U);
  tau_w(theta)   wall_shear(u, mu), positive along the traversal (clockwise
                 round the obstacle);
  separation     the angles at which tau_w changes sign (crossings);
  forces         integrate(traction) summed, next to KarmanProblem.forces().

theta is the angle about the circle's centre in degrees, 180 = the side that
faces the inflow.  `--rows` samples are printed, evenly spaced along the curve.

Time of P.evaluate: 2 warm-up calls, then the median (min - max) of 7 windows
of `--batch` calls back to back between two HIP events, for Cp (one P1 field),
tau_w (a P2 vector field) and the traction (two outputs), on the obstacle and
on the whole boundary.

    python tools/profile_lab.py [--mesh NX NY] [--steps 0] [--degree 2]
                                [--rows 24] [--batch 20]
'''
import argparse
import math
import os
import sys
import time

import numpy
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from flow_amd import fem, device, karman        # noqa: E402


def timed(call, warmup=2, repeat=7, batch=20):
    '''ms per call: `batch` calls back to back between two events (one launch
    alone is a few microseconds: that would time the events), median, min and
    max of `repeat` such windows.'''
    for _ in range(warmup):
        call()
    device.synchronize()
    ms = []
    for _ in range(repeat):
        a, b = torch.cuda.Event(enable_timing=True), \
            torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(batch):
            call()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / batch)
    return numpy.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--mesh', type=int, nargs=2, default=[2182, 509])
    ap.add_argument('--steps', type=int, default=0)
    ap.add_argument('--degree', type=int, default=2)
    ap.add_argument('--rows', type=int, default=24)
    ap.add_argument('--batch', type=int, default=20)
    args = ap.parse_args()
    t0 = time.perf_counter()
    problem = karman.KarmanProblem(args.mesh[0], args.mesh[1])
    problem.set_initial_stokes()
    for _ in range(args.steps):
        problem.step()
    mesh = problem.mesh
    print('mesh %d x %d: %d cells, %d boundary facets; Stokes start + %d steps, '
          't = %.3e (%.1f s)'
          % (args.mesh[0], args.mesh[1], mesh.num_cells(), len(mesh.bfacets),
             args.steps, problem.t, time.perf_counter() - t0), flush=True)
    cx, cy, r = mesh.hole
    t0 = time.perf_counter()
    P = fem.BoundaryProfile(mesh, karman.ObstacleBoundary(problem.length),
                            degree=args.degree, start=(cx - r, cy))
    print('obstacle: %d curve(s), %d facets, %d samples, length %.6f '
          '(2 pi r = %.6f) (set-up %.2f s)'
          % (P.num_curves, P.nfacets, P.npoints, P.curve_length(0),
             2 * math.pi * r, time.perf_counter() - t0), flush=True)
    u, p, mu, rho = problem.u0, problem.p0, problem.mu, problem.rho
    U = karman.ENTRANCE_VELOCITY
    p_front = float(device.to_host(P.evaluate(p))[0, 0])
    cp_expr = fem.pressure_coefficient(p, p_front, rho, U)
    tau_expr = fem.wall_shear(u, mu)
    trac_expr = fem.traction(u, p, mu)
    cp = device.to_host(P.evaluate(cp_expr)).numpy()[0]
    tau = device.to_host(P.evaluate(tau_expr)).numpy()[0]
    theta = numpy.degrees(P.angle((cx, cy))) % 360.0
    print('%10s %10s %12s %14s' % ('s', 'theta', 'Cp', 'tau_w'))
    for i in numpy.linspace(0, P.npoints - 1, min(args.rows, P.npoints)).astype(int):
        print('%10.6f %10.3f %12.5f %14.6e' % (P.s[i], theta[i], cp[i], tau[i]))
    at, = P.crossings(tau)
    ang = [float(numpy.interp(s, P.s, numpy.unwrap(numpy.radians(theta))))
           for s in at]
    print('tau_w changes sign at s = %s, theta = %s degrees'
          % (', '.join('%.6f' % s for s in at),
             ', '.join('%.2f' % (math.degrees(a) % 360.0) for a in ang)))
    total = device.to_host(P.total(trac_expr)).numpy()[:, 0]
    want = problem.forces()
    print('drag %.9e (forces(): %.9e)  lift %.9e (forces(): %.9e)'
          % (total[0], want['drag'], total[1], want['lift']), flush=True)
    whole = fem.BoundaryProfile(mesh, degree=args.degree)
    for name, Q in (('obstacle', P), ('whole boundary', whole)):
        print('%s: %d facets, %d samples' % (name, Q.nfacets, Q.npoints))
        for what, expr in (('Cp', cp_expr), ('tau_w', tau_expr),
                           ('traction', trac_expr)):
            out = Q.evaluate(expr)
            med, lo, hi = timed(lambda: Q.evaluate(expr, out=out),
                                batch=args.batch)
            print('    evaluate %-9s %8.2f us (%.2f - %.2f)'
                  % (what, 1e3 * med, 1e3 * lo, 1e3 * hi), flush=True)
        out = Q.cumulative(trac_expr)
        med, lo, hi = timed(lambda: Q.cumulative(trac_expr), batch=args.batch)
        print('    cumulative traction %6.2f us (%.2f - %.2f)'
              % (1e3 * med, 1e3 * lo, 1e3 * hi), flush=True)


if __name__ == '__main__':
    main()
