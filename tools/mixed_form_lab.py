# -*- coding: utf-8 -*-
'''
Mixed forms on a Taylor-Hood space ("Mixed forms"): what
assembly, the block-wise product and one MINRES iteration cost, on the P2/P1
space of the body-fitted Karman channel karman_channel(nx, ny, fitted=True)
(default 1035 x 241: about 0.5 M cells, 2.2 M unknowns) with the reference's
form

    a = mu*inner(grad(u), grad(v))*dx - p*div(v)*dx - q*div(u)*dx

  assemble        assemble(a) as a user calls it -- programs compiled, five
                  block launches, the gathers --: a host clock around the call
                  and a device synchronise, so the Python of the call counts.
                  assemble_system(a, L, bcs) likewise (it adds the symmetric
                  part, the lift and the elimination).
  apply           MixedMatrix.apply whole, and one flow_operator_apply per
                  present block (uu, up0, up1, pu0, pu1), HIP events around
                  `batch` calls back to back.  Bytes in the traffic model: 12
                  nnz per scalar plane (values and columns; uu reads its
                  columns once for four planes: 36 nnz), the row pointers, 8
                  bytes gathered per nonzero (mostly from cache) and 8 per row
                  written.  The sum of the blocks against the whole call is
                  the cost of composing the product from existing launches
                  (the axpby passes and the temporaries); the two planes of a
                  coupling pair share one pattern, and a product fused over it
                  -- not built -- would read the columns once for both.
  MINRES          mixed.minres for a fixed number of iterations (it stops with
                  NotConverged, which is caught) with the 'jacobi' and the
                  'two_level' velocity preconditioner: host clock with a
                  synchronise over the whole loop, per iteration.  The loop is
                  host driven and reads two dots back per iteration, so this
                  is an end-to-end figure, not a kernel time.

3 warm-ups, then the median of 7 windows with min - max.

    python tools/mixed_form_lab.py [NX [NY]] [--iterations K]
'''
import argparse
import os
import sys
import time

import numpy
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from flow_amd import fem, device, _hip               # noqa: E402
from flow_amd.fem import (                           # noqa: E402
    TestFunctions, TrialFunctions, assemble, assemble_system, dx, inner, grad,
    div, mixed,
    )


def timed(call, warmup=3, repeat=7, batch=10):
    '''(median, min, max) ms per call: HIP events around `batch` calls.'''
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


def walled(call, warmup=3, repeat=7):
    '''(median, min, max) ms per call: a host clock around the call and a
    device synchronise (the Python of the call counts).'''
    for _ in range(warmup):
        call()
    device.synchronize()
    ms = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        call()
        device.synchronize()
        ms.append(1.0e3 * (time.perf_counter() - t0))
    return numpy.median(ms), min(ms), max(ms)


def block_bytes(name, B):
    '''Bytes one product of a block moves in the traffic model.'''
    if name == 'uu':
        lay = B.layout
        return 36 * lay.nnz + 4 * (lay.N + 1) + 4 * 8 * lay.nnz + 16 * lay.N
    if name == 'pp':
        lay = B.layout
        return 12 * lay.nnz + 4 * (lay.N + 1) + 8 * lay.nnz + 8 * lay.N
    lay = B.layout
    return 12 * lay.nnz + 4 * (lay.shape[0] + 1) + 8 * lay.nnz \
        + 8 * lay.shape[0]


def problem(nx, ny):
    mesh = fem.karman_channel(nx, ny, fitted=True)
    WP = fem.FunctionSpace(
        mesh, fem.VectorElement('Lagrange', 'triangle', 2)
        * fem.FiniteElement('Lagrange', 'triangle', 1))
    (u, p), (v, q) = TrialFunctions(WP), TestFunctions(WP)
    mu = fem.Constant(0.002)
    a = mu * inner(grad(u), grad(v)) * dx - p * div(v) * dx \
        - q * div(u) * dx
    L = inner(fem.Constant((0.0, 0.0)), v) * dx
    (x0, y0), (x1, y1) = mesh.points.min(axis=0), mesh.points.max(axis=0)

    class Side(fem.SubDomain):
        def __init__(self, test):
            fem.SubDomain.__init__(self)
            self.test = test

        def inside(self, x, on_boundary):
            return on_boundary & self.test(x)

    inflow = fem.Expression(
        ('4.0*x[1]*(H - x[1])/(H*H)', '0.0'), degree=2, H=float(y1 - y0))
    bcs = [
        # (walls and the cylinder: everything on the boundary but the outlet;
        # the inflow profile, set afterwards, wins on the inlet)
        fem.DirichletBC(WP.sub(0), fem.Constant((0.0, 0.0)),
                        Side(lambda x: x[0] < x1 - 1e-12)),
        fem.DirichletBC(WP.sub(0), inflow, Side(lambda x: x[0] < x0 + 1e-12)),
        ]
    return mesh, WP, a, L, bcs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('nx', nargs='?', type=int, default=1035)
    ap.add_argument('ny', nargs='?', type=int, default=None)
    ap.add_argument('--iterations', type=int, default=20)
    args = ap.parse_args()
    ny = args.ny if args.ny is not None else int(round(args.nx * 509.0 / 2182.0))
    with fem.mixed_arguments(True), fem.vector_arguments(True):
        mesh, WP, a, L, bcs = problem(args.nx, ny)
        W, P = WP.sub(0), WP.sub(1)
        print('karman_channel(%d, %d, fitted): %d cells, 2 x %d + %d = %d '
              'unknowns' % (args.nx, ny, mesh.num_cells(), W.N, P.N,
                            WP.size()))
        _hip.lib()
        t = walled(lambda: assemble(a))
        print('assemble(a):               %8.3f ms (%.3f - %.3f)' % t)
        t = walled(lambda: assemble_system(a, L, bcs))
        print('assemble_system(a, L, bcs): %8.3f ms (%.3f - %.3f)' % t)

        masks = {}
        A, b = mixed.assemble_system(a, L, bcs, None, masks)
        x, y = device.zeros(A.size) + 1.0, device.empty(A.size)
        nv, n2 = W.N, W.size()
        whole = timed(lambda: A.apply(x, y))
        print('MixedMatrix.apply:         %8.3f ms (%.3f - %.3f)' % whole)
        total = 0.0
        for name, B in A.blocks():
            if name == 'uu':
                call = (lambda B=B: B.apply(x[:n2], y[:n2]))
            elif name == 'pp':
                call = (lambda B=B: B.apply(x[n2:], y[n2:]))
            elif name.startswith('up'):
                call = (lambda B=B: B.apply(x[n2:], y[:nv]))
            else:
                call = (lambda B=B: B.apply(x[:nv], y[n2:]))
            t = timed(call)
            total += t[0]
            nbytes = block_bytes(name, B)
            print('  block %-3s %10d nnz: %8.3f ms (%.3f - %.3f), %6.1f MB in '
                  'the model, %7.1f GB/s'
                  % ((name, B.layout.nnz) + tuple(t)
                     + (nbytes / 1e6, nbytes / t[0] / 1e6)))
        print('  sum of the blocks %.3f ms; the whole call / the sum %.2f'
              % (total, whole[0] / total))

        for velocity in ('jacobi', 'two_level'):
            pdiag = mixed._schur_diagonal(A, masks['p'])
            M = mixed.BlockPreconditioner(A, velocity, pdiag, masks['u'])

            def loop():
                w = device.zeros(A.size)
                try:
                    mixed.minres(A.apply, M.apply, b.data, w, 1.0e-30,
                                 maxit=args.iterations)
                except _hip.NotConverged:
                    pass

            t = walled(loop)
            print('MINRES, %-9s: %8.3f ms per iteration (%.3f - %.3f), %d '
                  'iterations per window'
                  % ((velocity,) + tuple(v / args.iterations for v in t)
                     + (args.iterations,)))


if __name__ == '__main__':
    main()
