# -*- coding: utf-8 -*-
'''
Cost of fem.Transfer ("Field transfer"): a P2 vector
field from the fitted channel karman_channel(nx_from, ny_from) to the bench
mesh karman_channel(2182, 509), with extrapolation.

  construction  Transfer(...): upload of the nodes, flow_locate_points,
                flow_nearest_cells, the read-backs (wall clock: it
                synchronises);
  apply         flow_transfer_apply, one launch for both components;
  probes        the same values through Probes(mesh_from, nodes).evaluate(u):
                flow_form_points, the form interpreter at one wave per SIMD --
                the only path before Transfer (NaN at the nodes outside).

HIP events, 2 warm-up calls, median of 7 with min and max.  Prints the
effective traffic of apply (cell, bary, out streams and 6 source values per
node and component) and the largest difference between the two paths.

    python tools/transfer_lab.py [nx [ny]] [--from NX_FROM]
'''
import os
import sys
import time

import numpy
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from flow_amd import fem, device       # noqa: E402


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


def main():
    args = sys.argv[1:]
    nx_from = None
    if '--from' in args:
        i = args.index('--from')
        nx_from = int(args[i + 1])
        del args[i:i + 2]
    nx = int(args[0]) if args else 2182
    ny = int(args[1]) if len(args) > 1 else int(round(nx * 509.0 / 2182.0))
    if nx_from is None:
        nx_from = nx // 2
    src = fem.karman_channel(nx_from, fitted=True)
    dst = fem.karman_channel(nx, ny, fitted=True)
    V_from = fem.VectorFunctionSpace(src, 'CG', 2)
    V_to = fem.VectorFunctionSpace(dst, 'CG', 2)
    u = fem.interpolate(fem.Expression(('sin(20*x[0])*x[1] + 1.0',
                                        'cos(15*x[1])*x[0] - 0.5'), degree=2),
                        V_from)
    print('from %d cells (%d nodes) to %d cells (%d nodes), P2 vector'
          % (src.num_cells(), V_from.N, dst.num_cells(), V_to.N))
    fem.Probes(src, [(0.3, 0.0)])           # the source's point grid: built once
    device.synchronize()
    t0 = time.perf_counter()
    T = fem.Transfer(V_from, V_to, allow_extrapolation=True)
    device.synchronize()
    t1 = time.perf_counter()
    print('construction           %9.3f ms wall; %d of %d nodes outside, '
          'farthest %.3e' % (1e3 * (t1 - t0), (~T.found).sum(), T.n,
                             T.distance.max()))
    w = fem.Function(V_to)
    ap = timed(lambda: T.apply(u, out=w))
    n = T.n
    traffic = n * (4 + 3 * 8 + 2 * 8 + 6 * 4 + 2 * 6 * 8)
    print('apply                  %9.3f ms (%.3f - %.3f)   %.1f GB/s of %d '
          'bytes per node' % (ap + (1e-6 * traffic / ap[0], traffic // n)))
    probes = fem.Probes(src, V_to.layout.dof_coords)
    out = device.empty(2 * n).view(2, n)
    pr = timed(lambda: probes.evaluate(u, out=out))
    print('Probes.evaluate        %9.3f ms (%.3f - %.3f)' % pr)
    print('Probes.evaluate / apply: %.2f' % (pr[0] / ap[0]))
    a = w.array().reshape(2, n)
    b = device.to_host(out).numpy()
    f = T.found
    print('max |difference| at the nodes inside: %.2e (max |u| %.2e)'
          % (numpy.abs(a[:, f] - b[:, f]).max(), numpy.abs(a).max()))


if __name__ == '__main__':
    main()
