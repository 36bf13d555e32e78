#!/usr/bin/env python
# -*- coding: utf-8 -*-
'''
What dx(k) costs: assemble() of a P2 stiffness form over cell subdomains that
hold about 5 %, 50 % and 100 % of the cells of the fitted Karman channel,
against the same form over plain dx.

    python tools/cell_subdomain_lab.py [--nx 400] [--ny 92] [--repeat 7]

Needs the GPU: without one it fails, it does not fall back.  Every variant is
warmed up (code objects, the cached cell list and contribution map), then
timed `repeat` times in alternation with the others; a timing is a host clock
around `calls` assemblies that ends in a device synchronise, with `calls`
chosen so that a window lasts about a second.  Reported per call:
minimum, median and maximum over the repeats, and the ratio of the medians to
plain dx.  The assembled values of the 100 % selection are compared with
plain dx bit for bit.  No test asserts a time.
'''
import argparse
import os
import sys
import time

import numpy

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from flow_amd import device, fem, _hip                      # noqa: E402
from flow_amd.fem import (                                  # noqa: E402
    TestFunction, TrialFunction, assemble, dx, Measure, MeshFunction, inner,
    grad,
    )


def _sync():
    import torch
    torch.cuda.synchronize()


def _window(fn, calls):
    _sync()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    _sync()
    return (time.perf_counter() - t0) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nx', type=int, default=400)
    ap.add_argument('--ny', type=int, default=92)
    ap.add_argument('--repeat', type=int, default=7)
    ap.add_argument('--window', type=float, default=1.0,
                    help='seconds per timed window')
    args = ap.parse_args()
    if not device.on_gpu():
        raise SystemExit('cell_subdomain_lab: no GPU; nothing is measured '
                         'without one')
    _hip.lib()
    with fem.cell_subdomains(True):
        mesh = fem.karman_channel(args.nx, args.ny, fitted=True)
        nc = mesh.num_cells()
        V = fem.FunctionSpace(mesh, 'CG', 2)
        u, v = TrialFunction(V), TestFunction(V)
        kappa = fem.Constant(2.5)
        # cells by their midpoint's x: a strip that holds the wanted share
        x = mesh.points[mesh.cell_vertices].mean(axis=1)[:, 0]
        order = numpy.argsort(x, kind='stable')
        variants = [('dx', kappa * inner(grad(u), grad(v)) * dx(mesh), nc)]
        for share in (0.05, 0.5, 1.0):
            m = MeshFunction('size_t', mesh, 2, 0)
            chosen = numpy.zeros(nc, dtype=bool)
            chosen[order[:max(1, int(round(share * nc)))]] = True
            m.set_where(chosen, 1)
            d = Measure('dx', domain=mesh, subdomain_data=m)(1)
            variants.append(('dx(k) %3.0f %%' % (100 * share),
                             kappa * inner(grad(u), grad(v)) * d,
                             int(chosen.sum())))
        print('fitted Karman channel %d x %d: %d cells, P2, %d dofs, %d '
              'nonzeros' % (args.nx, args.ny, nc, V.N, V.layout.nnz))
        same = numpy.array_equal(
            assemble(variants[0][1]).plane(0).cpu().numpy(),
            assemble(variants[3][1]).plane(0).cpu().numpy())
        print('dx(k) over every cell has the bits of dx: %s' % same)
        calls = []
        for name, form, n in variants:
            fn = lambda form=form: assemble(form)            # noqa: E731
            for _ in range(3):
                fn()
            t = _window(fn, 5)
            calls.append(max(5, int(args.window / t)))
        times = [[] for _ in variants]
        for _ in range(args.repeat):
            for i, (name, form, n) in enumerate(variants):
                times[i].append(_window(lambda: assemble(form), calls[i]))
        base = numpy.median(times[0])
        print('%-14s %9s %7s %11s %11s %11s %8s'
              % ('variant', 'cells', 'calls', 'min [us]', 'median [us]',
                 'max [us]', 'vs dx'))
        for (name, form, n), t, c in zip(variants, times, calls):
            t = numpy.array(t) * 1e6
            print('%-14s %9d %7d %11.1f %11.1f %11.1f %8.3f'
                  % (name, n, c, t.min(), numpy.median(t), t.max(),
                     numpy.median(t) / (base * 1e6)))


if __name__ == '__main__':
    main()
