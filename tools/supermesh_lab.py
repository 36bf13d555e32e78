# -*- coding: utf-8 -*-
'''
Cost of fem.Projection ("Conservative transfer"): a P2
vector field from the fitted channel karman_channel(nx, ny) -- the bench
mesh at the default size -- to a once-refined copy of it (fem.refine, every
cell) and back.

  pairs         candidate source cells per target cell (mean, max), and the
                wall time of the host's pair list;
  construction  Projection(...): pair list, upload, the geometry launch, the
                read-back of the coverage (wall clock: it synchronises);
  load          flow_project_load: the supermesh kernel and the gather;
  apply         load and the two mass solves (for scale: what the transfer
                step of an adaptive loop costs);
  Transfer      Transfer.apply between the same spaces: interpolation, the
                cheapest possible transfer.

HIP events, 2 warm-up calls, median of 7 with min and max.  (tools/
projection_lab.py is another lab: projection onto earlier solutions as a
start vector.)

    python tools/supermesh_lab.py [nx [ny]]
'''
import os
import sys
import time

import numpy
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from flow_amd import fem, device       # noqa: E402
from flow_amd.fem import projection    # noqa: E402


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


def one_way(what, V_from, V_to, u):
    t0 = time.perf_counter()
    pptr, _ = projection.pair_list(V_from.mesh(), V_to.mesh())
    t1 = time.perf_counter()
    per = numpy.diff(pptr)
    print('%s: %d -> %d cells; pairs per target cell: mean %.2f, max %d; '
          'pair list %.2f s on the host'
          % (what, V_from.mesh().num_cells(), V_to.mesh().num_cells(),
             per.mean(), per.max(), t1 - t0))
    device.synchronize()
    t0 = time.perf_counter()
    P = fem.Projection(V_from, V_to, allow_partial=True)
    device.synchronize()
    t1 = time.perf_counter()
    print('  construction         %9.3f s wall; min coverage %.15f'
          % (t1 - t0, P.min_coverage))
    print('  load                 %9.3f ms (%.3f - %.3f)'
          % timed(lambda: P.load(u)))
    w = fem.Function(V_to)
    print('  apply                %9.3f ms (%.3f - %.3f)'
          % timed(lambda: P.apply(u, out=w)))
    T = fem.Transfer(V_from, V_to, allow_extrapolation=True)
    v = fem.Function(V_to)
    print('  Transfer.apply       %9.3f ms (%.3f - %.3f)'
          % timed(lambda: T.apply(u, out=v)))
    return w


def main():
    args = sys.argv[1:]
    nx = int(args[0]) if args else 2182
    ny = int(args[1]) if len(args) > 1 else int(round(nx * 509.0 / 2182.0))
    coarse = fem.karman_channel(nx, ny, fitted=True)
    fine = fem.refine(coarse)
    V_c = fem.VectorFunctionSpace(coarse, 'CG', 2)
    V_f = fem.VectorFunctionSpace(fine, 'CG', 2)
    u = fem.interpolate(fem.Expression(('sin(20*x[0])*x[1] + 1.0',
                                        'cos(15*x[1])*x[0] - 0.5'), degree=2),
                        V_c)
    w = one_way('coarse -> fine', V_c, V_f, u)
    back = one_way('fine -> coarse', V_f, V_c, w)
    print('there and back: max |difference| %.2e (max |u| %.2e)'
          % (numpy.abs(back.array() - u.array()).max(), numpy.abs(u.array()).max()))


if __name__ == '__main__':
    main()
