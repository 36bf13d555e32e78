# -*- coding: utf-8 -*-
'''
Newton's method on a Taylor-Hood space ("Mixed Newton";
fem.mixed_derivatives): what the first half of the block-triangular
preconditioner costs composed and in one launch, and what one Newton step
costs.

  preconditioner  BlockTriangularPreconditioner.apply (a vmul, a copy, per
            coupling plane a product and an axpby, then the ILU(0) sweeps)
            against apply_fused (flow_mixed_upper_rhs, then the same sweeps) on
            the Navier-Stokes Jacobian of the P2/P1 space of
            karman_channel(nx, ny, fitted=True) (default 1035 x 241: 2.2 M
            unknowns) at the Poiseuille profile: HIP events around `batch`
            calls back to back, 3 warm-ups, then 7 windows of each, the two
            ALTERNATING window by window in one process; medians with min -
            max, and the ratio.  The same for the first halves alone (without
            the sweeps) and for the 'jacobi' velocity part.  The results are
            compared bit for bit first.
  Newton step     MixedNewtonAssembler.assemble + system (the frozen blocks
            are assembled once, before the clock), the preconditioner's
            refresh, and mixed.fgmres for a fixed number of iterations (it
            stops with NotConverged, which is caught) over apply and over
            apply_fused: a host clock with a synchronise, medians of 7.  Host
            driven: an end-to-end figure, not a kernel time.

    python tools/mixed_newton_lab.py [NX [NY]] [--iterations K]
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
    TestFunctions, derivative, dx, dot, inner, grad, div, mixed, ops,
    )
from mixed_form_lab import walled, problem           # noqa: E402
from oseen_lab import timed_alternating              # noqa: E402


def lab(nx, ny, iterations):
    mesh, WP, _, _, bcs = problem(nx, ny)
    W, P = WP.sub(0), WP.sub(1)
    print('karman_channel(%d, %d, fitted): %d cells, 2 x %d + %d = %d unknowns'
          % (nx, ny, mesh.num_cells(), W.N, P.N, WP.size()))
    (x0, y0), (x1, y1) = mesh.points.min(axis=0), mesh.points.max(axis=0)
    w = fem.Function(WP)
    vals = numpy.zeros(WP.size())
    y = W.layout.dof_coords[:, 1]
    vals[:W.N] = 4.0 * (y - y0) * (y1 - y) / (y1 - y0) ** 2
    w.set_array(vals)
    (u, p), (v, q) = fem.split(w), TestFunctions(WP)
    F = fem.Constant(0.002) * inner(grad(u), grad(v)) * dx \
        + dot(dot(grad(u), u), v) * dx - p * div(v) * dx - q * div(u) * dx \
        - inner(fem.Constant((0.0, 0.0)), v) * dx
    asm = mixed.MixedNewtonAssembler(derivative(F, w), F, WP, w=w)
    print('frozen blocks: %s' % (asm.frozen,))
    held = mixed.mixed_bcs(bcs, WP)
    um, pm = device.to_device(held[2]), device.to_device(held[3])
    asm.assemble()
    A = asm.system(um, pm)
    b = asm.b
    rng = numpy.random.RandomState(0)
    r = device.to_device(rng.standard_normal(A.size))
    za, zf = device.empty(A.size), device.empty(A.size)
    n2 = W.size()
    decisions = {}
    for velocity in ('ilu0', 'jacobi'):
        M = mixed.BlockTriangularPreconditioner(A, velocity)
        M.apply(r, za)
        M.apply_fused(r, zf)
        same = bool(torch.equal(za, zf))
        print('%s: apply_fused == apply bit for bit: %s' % (velocity, same))
        assert same
        composed, fused = timed_alternating(
            [lambda: M.apply(r, za), lambda: M.apply_fused(r, zf)])
        print('%-6s apply:        %8.4f ms (%.4f - %.4f)'
              % ((velocity,) + composed))
        print('%-6s apply_fused:  %8.4f ms (%.4f - %.4f)'
              % ((velocity,) + fused))
        print('%-6s apply / apply_fused: %.3f' % (velocity,
                                                   composed[0] / fused[0]))
        decisions[velocity] = fused[0] <= composed[0]
    # the first halves alone
    M = mixed.BlockTriangularPreconditioner(A, 'jacobi')
    tmp = device.empty(W.N)
    nv = W.N

    def first_half():
        ops.vmul(r[n2:], M.sinv, za[n2:])
        ru = ops.copy(M.ru, r[:n2])
        for c in range(2):
            A.up[c].apply(za[n2:], tmp)
            ops.axpby(-1.0, tmp, 1.0, ru[c * nv:(c + 1) * nv])

    ru2 = device.empty(n2)
    composed, fused = timed_alternating(
        [first_half, lambda: mixed.upper_rhs(A, M.sinv, r, zf[n2:], ru2)])
    print('first half composed (6 launches): %8.4f ms (%.4f - %.4f)' % composed)
    print('flow_mixed_upper_rhs (1 launch):  %8.4f ms (%.4f - %.4f)' % fused)
    print('composed / one launch:            %8.3f' % (composed[0] / fused[0]))
    print('Newton uses %s (the rule: apply_fused where its median is not above '
          "apply's, 'ilu0')" % ('apply_fused' if decisions['ilu0'] else 'apply'))

    # one Newton step
    def assemble():
        asm.assemble()
        asm.system(um, pm)

    t = walled(assemble)
    print('assemble + system (frozen blocks reused): %8.3f ms (%.3f - %.3f)' % t)
    M = mixed.BlockTriangularPreconditioner(A, 'ilu0')
    t = walled(lambda: M.refresh())
    print('preconditioner refresh (ILU(0) refactor, Schur diagonal): %8.3f ms '
          '(%.3f - %.3f)' % t)
    for name, prec in (('apply', M.apply), ('apply_fused', M.apply_fused)):
        def loop():
            d = device.zeros(A.size)
            try:
                mixed.fgmres(A.apply_fused, prec, b, d, 1.0e-30,
                             maxit=iterations, restart=iterations)
            except _hip.NotConverged:
                pass

        t = walled(loop)
        print('FGMRES over %-11s: %8.3f ms per iteration (%.3f - %.3f), %d '
              'iterations per window'
              % ((name,) + tuple(x / iterations for x in t) + (iterations,)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('nx', nargs='?', type=int, default=1035)
    ap.add_argument('ny', nargs='?', type=int, default=None)
    ap.add_argument('--iterations', type=int, default=20)
    args = ap.parse_args()
    ny = args.ny if args.ny is not None else int(round(args.nx * 509.0 / 2182.0))
    with fem.mixed_arguments(True), fem.vector_arguments(True), \
            fem.mixed_gmres(True), fem.mixed_derivatives(True):
        _hip.lib()
        lab(args.nx, ny, args.iterations)


if __name__ == '__main__':
    main()
