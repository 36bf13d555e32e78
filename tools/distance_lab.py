# -*- coding: utf-8 -*-
'''
The wall distance ("Wall distance"): what fem.Distance
costs on the bench mesh and how many sweeps go into one batch.

On the mesh of KarmanProblem(nx, ny) (default 2182 x 509: 1.1 M vertices),
sources = the obstacle, P1 and P2, for each batch size (the module constant
distance.CHECK_EVERY, set here from the list):

  apply ms     wall clock around D.apply(out=d) with the read-back of the flag
               behind every batch, ended by a device synchronisation; 2
               warm-up calls, median of 7 with min - max;
  sweeps       D.sweeps: what the fixed point needs, rounded up to the batch;
  us / sweep   the two divided, and GB/s by the traffic model of DESIGN.md.

The same bits for every batch size are asserted.

    python tools/distance_lab.py [--mesh NX NY] [--batches 8 32 128]
                                 [--degrees 1 2] [--repeat 7]
'''
import argparse
import os
import sys
import time

import numpy
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from flow_amd import fem, device, karman        # noqa: E402
from flow_amd.fem import distance                # noqa: E402


def timed(call, warmup=2, repeat=7):
    '''ms per call by the host's clock, each call ended by a synchronisation:
    median, min and max of `repeat` calls after `warmup`.'''
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


def traffic(V, nc):
    '''Bytes one sweep moves at least (DESIGN.md's model): per dof its row
    bounds, its old and new value; per entry of the map the entry, the cell's
    six coordinates and, per sub-triangle, two dof indices and two values.'''
    tri = nc * (3 if V.degree == 1 else 12)
    return V.N * (8 + 16) + V.layout.nloc * nc * (4 + 48) + tri * (8 + 16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--mesh', type=int, nargs=2, default=[2182, 509])
    ap.add_argument('--batches', type=int, nargs='+', default=[8, 32, 128])
    ap.add_argument('--degrees', type=int, nargs='+', default=[1, 2])
    ap.add_argument('--repeat', type=int, default=7)
    args = ap.parse_args()
    t0 = time.perf_counter()
    mesh = fem.karman_channel(args.mesh[0], args.mesh[1], fitted=True)
    nc = mesh.num_cells()
    print('mesh %d x %d: %d vertices, %d cells (%.1f s)'
          % (args.mesh[0], args.mesh[1], mesh.num_vertices(), nc,
             time.perf_counter() - t0), flush=True)
    for deg in args.degrees:
        V = fem.FunctionSpace(mesh, 'CG', deg)
        t0 = time.perf_counter()
        D = fem.Distance(V, karman.ObstacleBoundary())
        d = fem.Function(V)
        print('P%d: %d dofs, %d source dofs (set-up %.1f s)'
              % (deg, V.N, len(D.dofs), time.perf_counter() - t0), flush=True)
        first = None
        for every in args.batches:
            distance.CHECK_EVERY = every
            med, lo, hi = timed(lambda: D.apply(out=d), repeat=args.repeat)
            if first is None:
                first = d.data.clone()
                top = float(device.to_host(first.max()))
                print('    max d = %.6f' % top, flush=True)
            assert torch.equal(first, d.data), 'the batch size moved the bits'
            per = 1.0e3 * med / D.sweeps
            print('    CHECK_EVERY %4d: apply %9.2f ms (%.2f - %.2f), %5d '
                  'sweeps, %7.2f us / sweep, %7.1f GB/s'
                  % (every, med, lo, hi, D.sweeps, per,
                     traffic(V, nc) / per * 1.0e-3), flush=True)


if __name__ == '__main__':
    main()
