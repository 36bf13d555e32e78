# -*- coding: utf-8 -*-
'''
Non-symmetric mixed solves ("Non-symmetric mixed solves";
fem.mixed_gmres): steady Navier-Stokes by Picard iteration, and what the block
product and one FGMRES iteration cost.

  Picard    Kovasznay's flow at Re = 40 on [-0.5, 1] x [-0.5, 1.5] (RectangleMesh
            n x n, P2/P1), exact Dirichlet data, one pinned pressure dof, from a
            zero start: every step is the user's Oseen form with wu =
            split(w_old)[0], solved by solve(a == L, w, bcs).  Prints the FGMRES
            iterations of each step, the increment and the error against the
            exact fields.
  product   MixedMatrix.apply (composed of a launch per block and the axpby
            passes) against MixedMatrix.apply_fused (flow_mixed_apply, one
            launch) on the Oseen matrix of the P2/P1 space of
            karman_channel(nx, ny, fitted=True) (default 1035 x 241: 2.2 M
            unknowns): HIP events around `batch` calls back to back, 3 warm-ups,
            then 7 windows of each, the two ALTERNATING window by window in one
            process; medians with min - max, and the ratio.  The two results
            are compared bit for bit first.
  FGMRES    mixed.fgmres for a fixed number of iterations (it stops with
            NotConverged, which is caught) with the 'ilu0' and the 'jacobi'
            velocity preconditioner: a host clock with a synchronise over the
            whole loop, per iteration.  Host driven, three read-backs per
            iteration: an end-to-end figure, not a kernel time.

    python tools/oseen_lab.py [NX [NY]] [--iterations K] [--picard N] [--steps S]
'''
import argparse
import os
import sys

import numpy
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from flow_amd import fem, device, _hip               # noqa: E402
from flow_amd.fem import (                           # noqa: E402
    TestFunctions, TrialFunctions, solve, dx, dot, inner, grad, div, mixed,
    )
from flow_amd.fem.bcs import FixedDofsBC             # noqa: E402
from mixed_form_lab import walled, problem           # noqa: E402


def oseen(WP, nu, wu):
    (u, p), (v, q) = TrialFunctions(WP), TestFunctions(WP)
    return nu * inner(grad(u), grad(v)) * dx \
        + dot(dot(grad(u), wu), v) * dx - p * div(v) * dx - q * div(u) * dx


def picard(n, steps):
    re = 40.0
    lam = re / 2.0 - numpy.sqrt(re * re / 4.0 + 4.0 * numpy.pi ** 2)
    two_pi = 2.0 * numpy.pi
    mesh = fem.RectangleMesh(fem.Point(-0.5, -0.5), fem.Point(1.0, 1.5), n, n)
    WP = fem.FunctionSpace(
        mesh, fem.VectorElement('Lagrange', 'triangle', 2)
        * fem.FiniteElement('Lagrange', 'triangle', 1))
    W, P = WP.sub(0), WP.sub(1)
    ue = fem.Expression(
        ('1.0 - exp(lam*x[0])*cos(k*x[1])', 'lam/k*exp(lam*x[0])*sin(k*x[1])'),
        degree=4, lam=float(lam), k=float(two_pi))

    def pe(x):
        return 0.5 * (1.0 - numpy.exp(2.0 * lam * x[:, 0]))

    # one pinned pressure dof: the vertex at the lower left corner
    pin = int(numpy.abs(P.layout.dof_coords - [-0.5, -0.5]).sum(axis=1).argmin())
    bcs = [fem.DirichletBC(WP.sub(0), ue, 'on_boundary'),
           FixedDofsBC(WP.sub(1), [pin], pe(P.layout.dof_coords[[pin]]))]
    xu, xp = W.layout.dof_coords, P.layout.dof_coords
    exact_u = numpy.concatenate([
        1.0 - numpy.exp(lam * xu[:, 0]) * numpy.cos(two_pi * xu[:, 1]),
        lam / two_pi * numpy.exp(lam * xu[:, 0]) * numpy.sin(two_pi * xu[:, 1])])
    exact_p = pe(xp)
    (v, q) = TestFunctions(WP)
    L = inner(fem.Constant((0.0, 0.0)), v) * dx
    w_old, w = fem.Function(WP), fem.Function(WP)
    a = oseen(WP, fem.Constant(1.0 / re), fem.split(w_old)[0])
    n2 = W.size()
    print('Kovasznay, Re = 40, RectangleMesh %d x %d, P2/P1: %d unknowns'
          % (n, n, WP.size()))
    for step in range(steps):
        # (GMRES(30) stagnates on the first, Stokes-like steps: a longer basis)
        info = solve(a == L, w, bcs, solver_parameters={
            'krylov_solver': {'restart': 400, 'maximum_iterations': 4000}})
        x = w.array()
        inc = numpy.abs(x - w_old.array()).max()
        print('  Picard %2d: %-12s %4d iterations, increment %.2e, error u '
              '%.2e p %.2e (max norm, relative)'
              % (step + 1, info.method, info.iterations, inc,
                 numpy.abs(x[:n2] - exact_u).max() / numpy.abs(exact_u).max(),
                 numpy.abs(x[n2:] - exact_p).max() / numpy.abs(exact_p).max()))
        w_old.set_array(x)


def timed_alternating(calls, warmup=3, repeat=7, batch=10):
    '''[(median, min, max)] ms per call of each of `calls`: HIP events around
    `batch` calls, the calls taking turns window by window.'''
    for call in calls:
        for _ in range(warmup):
            call()
    device.synchronize()
    ms = [[] for _ in calls]
    for _ in range(repeat):
        for k, call in enumerate(calls):
            a, b = torch.cuda.Event(enable_timing=True), \
                torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(batch):
                call()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b) / batch)
    return [(numpy.median(m), min(m), max(m)) for m in ms]


def product_and_fgmres(nx, ny, iterations):
    mesh, WP, _, L, bcs = problem(nx, ny)
    W, P = WP.sub(0), WP.sub(1)
    print('karman_channel(%d, %d, fitted): %d cells, 2 x %d + %d = %d unknowns'
          % (nx, ny, mesh.num_cells(), W.N, P.N, WP.size()))
    (x0, y0), (x1, y1) = mesh.points.min(axis=0), mesh.points.max(axis=0)
    w0 = fem.Function(WP)
    vals = numpy.zeros(WP.size())
    y = W.layout.dof_coords[:, 1]
    vals[:W.N] = 4.0 * (y - y0) * (y1 - y) / (y1 - y0) ** 2
    w0.set_array(vals)
    a = oseen(WP, fem.Constant(0.002), fem.split(w0)[0])
    masks = {}
    A, b = mixed.assemble_system(a, L, bcs, None, masks)
    rng = numpy.random.RandomState(0)
    x = device.to_device(rng.standard_normal(A.size))
    ya, yf = device.empty(A.size), device.empty(A.size)
    A.apply(x, ya)
    A.apply_fused(x, yf)
    same = bool(torch.equal(ya, yf))
    print('apply_fused == apply bit for bit: %s' % same)
    assert same
    s = A.fused()
    print('tiles: %d velocity, %d pressure' % (s.nvtiles, s.nptiles))
    composed, fused = timed_alternating(
        [lambda: A.apply(x, ya), lambda: A.apply_fused(x, yf)])
    print('MixedMatrix.apply:        %8.4f ms (%.4f - %.4f)' % composed)
    print('MixedMatrix.apply_fused:  %8.4f ms (%.4f - %.4f)' % fused)
    print('apply / apply_fused:      %8.3f' % (composed[0] / fused[0]))
    sdiag = mixed._signed_schur_diagonal(A, masks['p'])
    for velocity in ('ilu0', 'jacobi'):
        M = mixed.BlockTriangularPreconditioner(A, velocity, sdiag)
        for name, product in (('apply_fused', A.apply_fused),
                              ('apply', A.apply)):
            def loop():
                w = device.zeros(A.size)
                try:
                    mixed.fgmres(product, M.apply, b.data, w, 1.0e-30,
                                 maxit=iterations, restart=iterations)
                except _hip.NotConverged:
                    pass

            t = walled(loop)
            print('FGMRES, %-6s over %-11s: %8.3f ms per iteration (%.3f - '
                  '%.3f), %d iterations per window'
                  % ((velocity, name) + tuple(v / iterations for v in t)
                     + (iterations,)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('nx', nargs='?', type=int, default=1035)
    ap.add_argument('ny', nargs='?', type=int, default=None)
    ap.add_argument('--iterations', type=int, default=20)
    ap.add_argument('--picard', type=int, default=16,
                    help='cells per side of the Kovasznay mesh (0: skip)')
    ap.add_argument('--steps', type=int, default=12, help='Picard steps')
    args = ap.parse_args()
    ny = args.ny if args.ny is not None else int(round(args.nx * 509.0 / 2182.0))
    with fem.mixed_arguments(True), fem.vector_arguments(True), \
            fem.mixed_gmres(True):
        _hip.lib()
        if args.picard:
            picard(args.picard, args.steps)
        if args.nx:
            product_and_fgmres(args.nx, ny, args.iterations)


if __name__ == '__main__':
    main()
